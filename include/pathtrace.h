// pathtrace.h — C++ mirror of the reference's hot-path boundary, src/pathtrace.h:6-9, with the
// reference's exact signatures.  Implemented (host/pathtrace_cpp.cpp) on top of the C-ABI in
// pt/pathtrace_abi.h; like the reference it keeps a non-owning Scene* and, on any device
// error, prints the error and exits (pathtrace.cu:27-49).
#pragma once

#include "pt/pathtrace_abi.h"
#include "scene.h"

void InitDataContainer(GuiDataContainer* guiData);
void pathtraceInit(Scene* scene);
void pathtraceFree();
void pathtrace(uchar4* pbo, int frame, int iteration);

// Framework addition: run-time replacement of the reference's compile-time switches
// (ERRORCHECK / STREAM_COMPACTION / MATERIAL_SORTING / BVH_ACCELERATION, pathtrace.cu:20-24).
// Takes effect at the next pathtraceInit.
void pathtraceSetOptions(const pt_options& opts);

// Framework addition: the accumulated image of the pathtrace() calls so far, divided by their
// count and passed through the edge-avoiding a-trous filter of pt/pt_denoise.h with its default
// parameters (feature buffer captured at iteration 1) -> out[width * height * 3].  The accumulated
// image itself is untouched.
void pathtraceDenoise(float* out);

// Framework addition: the reference's NAIVE_MESH_LOADING switch (pathtrace.cu:365-393) at run time,
// pt_set_naive_mesh of pt/pt_naive_mesh.h: every triangle in array order, no BVH.  Takes effect at
// the next pathtraceInit; options set through pathtraceSetOptions must then ask for
// PT_PIPELINE_STAGED (the defaults do).  The environment variable PT_NAIVE_MESH=1 does the same.
void pathtraceSetNaiveMesh(bool enabled);
