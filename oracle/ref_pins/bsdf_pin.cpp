// bsdf_pin.cpp — TEST INFRASTRUCTURE (oracle/_ref only; never shipped, never on the GPU box).
//
// Runs the reference's OWN shading math: src/interactions.cu (scatterRay and every BSDF helper,
// :7-542) and src/interactions.h, compiled in place as host C++ with g++ against the CUDA runtime
// headers and linked with this file.  Two things stand in for what a host build lacks:
//   * thrust/random.h is oracle/ref_pins/thrust_standin/thrust/random.h (minstd engine +
//     uniform_real_distribution<float>), itself pinned to rocThrust through
//     tests/golden/rng_pin.json;
//   * `-include math.h -include stdlib.h -include cuda_runtime.h`: with libstdc++'s math.h wrapper
//     the file's unqualified sqrt / cos / sin / abs on floats bind to the float overloads, which
//     is what nvcc gives the reference.  The static_asserts below fail the build otherwise.
// The only restated code is
//   * makeSeededRandomEngine (pathtrace.cu:51-56) with utilhash (intersections.h:13-22), as in
//     rng_pin.cpp, and
//   * of kernShadeMaterialProper (pathtrace.cu:521-621, a __global__ kernel that cannot be
//     compiled without nvcc) the three statements an untextured, non-emissive hit executes:
//     the seeding (:564), `intersect = ray.origin + ray.direction * t` in glm (:571) and the
//     scatterRay call (:609) with the record's normal and the scene's material.
// Textures and bump mapping (tex2D, :505-519, :549-552, :579-607), emissive hits, misses and
// finished paths are NOT restated: `shade` rejects such records.
//
// Modes (raw little-endian records):
//   bsdf_pin scatter <in> <out>          in : 9 f32 material (color[3], hasReflective, hasRefractive,
//                                             roughness, metallic, indexOfRefraction, emittance),
//                                             PathSegment (44 B), intersect[3], normal[3], i32 iter
//                                        out: PathSegment
//   bsdf_pin shade <scene.json> <in> <out>  in : ShadeableIntersection fields (t, normal[3], materialId,
//                                             uv[2], dpdu[3], dpdv[3]), PathSegment, i32 iter
//                                        out: PathSegment      (Scene from the reference's scene.cpp)
//   bsdf_pin materials <scene.json>      -> one line per material id: the nine floats above
#include "scene.h"
#include "interactions.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

// the float overloads must be the ones unqualified calls at global scope pick (see header comment)
static_assert(std::is_same<decltype(sqrt(1.f)), float>::value, "sqrt(float) must be float");
static_assert(std::is_same<decltype(cos(1.f)), float>::value, "cos(float) must be float");
static_assert(std::is_same<decltype(sin(1.f)), float>::value, "sin(float) must be float");
static_assert(std::is_same<decltype(abs(1.f)), float>::value, "abs(float) must be float");
static_assert(sizeof(PathSegment) == 44, "PathSegment layout");

namespace {

unsigned int utilhash(unsigned int a) {
    a = (a + 0x7ed55d16) + (a << 12);
    a = (a ^ 0xc761c23c) ^ (a >> 19);
    a = (a + 0x165667b1) + (a << 5);
    a = (a + 0xd3a2646c) ^ (a << 9);
    a = (a + 0xfd7046c5) + (a << 3);
    a = (a ^ 0xb55a4f09) ^ (a >> 16);
    return a;
}

// pathtrace.cu:51-56
thrust::default_random_engine makeSeededRandomEngine(int iter, int index, int depth) {
    int h = utilhash((1 << 31) | (depth << 22) | iter) ^ utilhash(index);
    return thrust::default_random_engine(h);
}

std::vector<char> slurp(const char* path) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::vector<char> raw;
    char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + n);
    std::fclose(f);
    return raw;
}

struct Reader {
    const char* p;
    template <class T> T get() { T v; std::memcpy(&v, p, sizeof(T)); p += sizeof(T); return v; }
    glm::vec3 v3() { float x = get<float>(), y = get<float>(), z = get<float>(); return glm::vec3(x, y, z); }
};

std::FILE* open_w(const char* p) {
    std::FILE* f = std::fopen(p, "wb");
    if (!f) { std::perror(p); std::exit(2); }
    return f;
}

const size_t SCATTER_REC = 9 * 4 + 44 + 12 + 12 + 4;
const size_t SHADE_REC = 52 + 44 + 4;

int scatter(const char* in_path, const char* out_path) {
    std::vector<char> raw = slurp(in_path);
    if (raw.size() % SCATTER_REC) { std::fprintf(stderr, "scatter: bad input size\n"); return 2; }
    std::FILE* f = open_w(out_path);
    Reader r{raw.data()};
    for (size_t i = 0; i < raw.size() / SCATTER_REC; ++i) {
        Material m{};
        m.color = r.v3();
        m.hasReflective = r.get<float>();
        m.hasRefractive = r.get<float>();
        m.roughness = r.get<float>();
        m.metallic = r.get<float>();
        m.indexOfRefraction = r.get<float>();
        m.emittance = r.get<float>();
        PathSegment ps = r.get<PathSegment>();
        glm::vec3 intersect = r.v3();
        glm::vec3 normal = r.v3();
        int iter = r.get<int>();
        thrust::default_random_engine rng = makeSeededRandomEngine(iter, ps.pixelIndex, ps.remainingBounces);
        scatterRay(ps, intersect, normal, m, rng);
        std::fwrite(&ps, sizeof ps, 1, f);
    }
    std::fclose(f);
    return 0;
}

int shade(const char* json, const char* in_path, const char* out_path) {
    Scene s(json);
    std::vector<char> raw = slurp(in_path);
    if (raw.size() % SHADE_REC) { std::fprintf(stderr, "shade: bad input size\n"); return 2; }
    std::FILE* f = open_w(out_path);
    Reader r{raw.data()};
    for (size_t i = 0; i < raw.size() / SHADE_REC; ++i) {
        float t = r.get<float>();
        glm::vec3 normal = r.v3();
        int materialId = r.get<int>();
        r.p += (2 + 3 + 3) * 4;                       // uv, dpdu, dpdv: textured paths only
        PathSegment ps = r.get<PathSegment>();
        int iter = r.get<int>();
        if (materialId < 0 || materialId >= (int)s.materials.size()) { std::fprintf(stderr, "shade: record %zu: material id\n", i); return 3; }
        Material material = s.materials[materialId];
        if (!(t > 0.0f) || ps.remainingBounces <= 0 || material.hasTexture || material.hasBumpMap ||
            material.emittance > 0.0f) {
            std::fprintf(stderr, "shade: record %zu is not an untextured, non-emissive hit\n", i);
            return 3;
        }
        thrust::default_random_engine rng = makeSeededRandomEngine(iter, ps.pixelIndex, ps.remainingBounces);
        Ray& ray = ps.ray;
        glm::vec3 intersect = ray.origin + ray.direction * t;
        scatterRay(ps, intersect, normal, material, rng);
        std::fwrite(&ps, sizeof ps, 1, f);
    }
    std::fclose(f);
    return 0;
}

int materials(const char* json) {
    Scene s(json);
    std::printf("BSDF_PIN_MATERIALS %zu\n", s.materials.size());
    for (const Material& m : s.materials)
        std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", m.color.x, m.color.y, m.color.z, m.hasReflective,
                    m.hasRefractive, m.roughness, m.metallic, m.indexOfRefraction, m.emittance);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "scatter" && argc == 4) return scatter(argv[2], argv[3]);
    if (mode == "shade" && argc == 5) return shade(argv[2], argv[3], argv[4]);
    if (mode == "materials" && argc == 3) return materials(argv[2]);
    std::fprintf(stderr, "usage: see header\n");
    return 2;
}
