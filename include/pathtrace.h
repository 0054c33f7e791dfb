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

// Framework addition: pathtraceDenoise with the blockwise feature regression of
// pt/pt_denoise_regress.h in place of the a-trous filter (default parameters, feature buffer captured
// at iteration 1) -> out[width * height * 3].  The accumulated image itself is untouched.
void pathtraceDenoiseRegress(float* out);

// Framework addition: pathtraceDenoise with the temporal stage of pt/pt_denoise_temporal.h in front
// (default parameters): the history of the earlier calls is reprojected through camera changes and
// a per-pixel variance guides the filter.  The feature buffer is captured when the camera changed
// since the last call; pathtraceInit / pathtraceFree drop the history.
void pathtraceDenoiseTemporal(float* out);

// Framework addition: the reference's NAIVE_MESH_LOADING switch (pathtrace.cu:365-393) at run time,
// pt_set_naive_mesh of pt/pt_naive_mesh.h: every triangle in array order, no BVH.  Takes effect at
// the next pathtraceInit; options set through pathtraceSetOptions must then ask for
// PT_PIPELINE_STAGED (the defaults do).  The environment variable PT_NAIVE_MESH=1 does the same.
void pathtraceSetNaiveMesh(bool enabled);
// Framework addition: primitive intersection through a 4-wide hierarchy over the geoms, pt_set_geom_bvh
// of pt/pt_geom_bvh.h (min_geoms <= 0: the default threshold, 65).  Takes effect at the next
// pathtraceInit; same images.  The environment variable PT_GEOM_BVH does the same.
void pathtraceSetGeomBvh(bool enabled, int min_geoms = 0);
