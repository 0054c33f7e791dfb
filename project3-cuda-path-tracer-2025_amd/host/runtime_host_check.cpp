// runtime_host_check.cpp — the runtime's pure host parts, stand-alone (no device code, no HIP):
//
//   runtime_host_check bands    band_layout.h: every shard's bands painted into a byte map of the image
//   runtime_host_check worker   worker.h: post / wait order, errors, restart after join, idle destructor
//   runtime_host_check tuning   tuning.h: defaults with no PT_* variable set, and clamped inputs
//   runtime_host_check          all three
//
// `make asan` builds it under AddressSanitizer + UndefinedBehaviorSanitizer, and under
// ThreadSanitizer where the compiler links it; tests/test_runtime_host.py runs them.  Exit status 0
// and a line "<part> ok" per part, or the first failed check and exit status 1.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "band_layout.h"
#include "tuning.h"
#include "worker.h"

extern char** environ;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            printf("FAILED %s: ", #cond);      \
            printf(__VA_ARGS__);               \
            printf("\n");                      \
            g_failed = 1;                      \
            return;                            \
        }                                      \
    } while (0)

// ---- band layout: every byte of the image covered exactly once, nothing past H rows ------------
void check_bands() {
    long cases = 0;
    for (int W : {1, 3})
        for (int H = 1; H <= 17; ++H)
            for (int rows = 1; rows <= 5; ++rows)
                for (int count = 1; count <= 4; ++count) {
                    const size_t bytes = 3 * sizeof(float) * (size_t)W * (size_t)H;
                    std::vector<unsigned char> map(bytes, 0);
                    auto paint = [&](size_t off, size_t n) {   // false: past the image's H rows
                        if (off > bytes || n > bytes - off) return false;
                        for (size_t i = 0; i < n; ++i) ++map[off + i];
                        return true;
                    };
                    for (int rank = 0; rank < count; ++rank) {
                        const pth::BandGeom g = pth::band_geometry(W, H, rows, count, rank);
                        for (size_t b = 0; b < g.height; ++b)
                            CHECK(paint(g.first + b * g.pitch, g.width), "W=%d H=%d rows=%d count=%d rank=%d band %zu past the image",
                                  W, H, rows, count, rank, b);
                        if (g.tail_bytes > 0)
                            CHECK(paint(g.tail_off, g.tail_bytes), "W=%d H=%d rows=%d count=%d rank=%d tail past the image", W, H,
                                  rows, count, rank);
                    }
                    for (size_t i = 0; i < bytes; ++i)
                        CHECK(map[i] == 1, "W=%d H=%d rows=%d count=%d: byte %zu covered %d times", W, H, rows, count, i,
                              (int)map[i]);
                    ++cases;
                }
    printf("bands ok cases=%ld\n", cases);
}

// ---- worker ----------------------------------------------------------------------------------
std::atomic<long> g_ran{0};
struct Echo {   // records its argument; an odd `fail` is its error
    int arg = 0, fail = 0;
    int* seen = nullptr;
    int run() const {
        if (seen) *seen = arg;
        ++g_ran;
        return fail;
    }
};

void check_worker() {
    {
        pth::Worker<Echo, int> idle;   // never started: the destructor returns
        pth::Worker<Echo, int, true> idle_sticky;
    }
    {
        pth::Worker<Echo, int> w;
        CHECK(w.wait() == 0, "wait() before any post");
        for (int i = 1; i <= 1000; ++i) {   // each round: this job's argument seen, this job's result back
            int seen = 0;
            w.post(Echo{i, i % 7 == 0 ? i : 0, &seen});
            const int e = w.wait();
            CHECK(seen == i, "round %d saw %d", i, seen);
            CHECK(e == (i % 7 == 0 ? i : 0), "round %d returned %d", i, e);
        }
        CHECK(g_ran == 1000, "ran %ld jobs", g_ran.load());
        // an error is returned once, then cleared
        w.post(Echo{1, 5, nullptr});
        CHECK(w.wait() == 5, "error not returned");
        CHECK(w.wait() == 0, "error returned twice");
        // join, then a new post restarts the thread
        w.join();
        int seen = 0;
        w.post(Echo{77, 0, &seen});
        CHECK(w.wait() == 0 && seen == 77, "after join: saw %d", seen);
        w.join();
        w.join();   // twice is harmless
        w.post(Echo{78, 3, &seen});
        CHECK(w.wait() == 3 && seen == 78, "after the second join: saw %d", seen);
    }
    {
        // the sticky form, used as its caller does (one wait between posts): the same answers
        pth::Worker<Echo, int, true> w;
        int seen = 0;
        w.post(Echo{1, 9, &seen});
        CHECK(w.wait() == 9 && seen == 1, "sticky: error not returned");
        CHECK(w.wait() == 0, "sticky: error returned twice");
        w.post(Echo{2, 0, &seen});
        CHECK(w.wait() == 0 && seen == 2, "sticky: a clean job after a read error");
        w.post(Echo{3, 4, nullptr});   // left unread: the destructor joins a started worker
    }
    printf("worker ok\n");
}

// ---- tuning ----------------------------------------------------------------------------------
void clear_pt_env() {
    std::vector<std::string> names;
    for (char** e = environ; e && *e; ++e)
        if (strncmp(*e, "PT_", 3) == 0) names.emplace_back(*e, strcspn(*e, "="));
    for (const std::string& n : names) unsetenv(n.c_str());
}

void check_tuning() {
    clear_pt_env();
    const pth::Tuning d, t = pth::read_tuning();
#define SAME(f) CHECK(t.f == d.f, "default of " #f " differs: %lld vs %lld", (long long)t.f, (long long)d.f)
    SAME(bounce_lds_pad); SAME(bvh_lds_pad); SAME(sections_skip_camera); SAME(tail_off); SAME(tail_any_batch);
    SAME(tail_from); SAME(head_fuse); SAME(auto_paths); SAME(f1_graph); SAME(multi_f1_direct); SAME(bvh_tail_lanes);
    SAME(bvh_tail_chunks); SAME(tail_refill); SAME(tail_trav_blocks); SAME(tail_shade_blocks);
    SAME(combine_force_staged); SAME(bvh_tree_ref); SAME(bvh_tree_info); SAME(bvh_max_height); SAME(bvh_quad);
    SAME(bvh_stack_lds); SAME(bvh_bfs_levels); SAME(grid); SAME(speculate); SAME(band_copy);
#undef SAME
    struct Case {
        const char* name;
        const char* value;
        long long (*get)(const pth::Tuning&);
        long long want;
    };
    const Case cases[] = {
        {"PT_BVH_TAIL_LANES", "99", [](const pth::Tuning& x) { return (long long)x.bvh_tail_lanes; }, 56},
        {"PT_BVH_TAIL_LANES", "-5", [](const pth::Tuning& x) { return (long long)x.bvh_tail_lanes; }, -1},
        {"PT_BVH_TAIL_REFILL", "0", [](const pth::Tuning& x) { return (long long)x.tail_refill; }, 1},
        {"PT_BVH_TAIL_REFILL", "1000", [](const pth::Tuning& x) { return (long long)x.tail_refill; }, 64},
        {"PT_BAND_COPY", "7", [](const pth::Tuning& x) { return (long long)x.band_copy; }, 1},
        {"PT_BAND_COPY", "-7", [](const pth::Tuning& x) { return (long long)x.band_copy; }, -1},
        {"PT_BVH_TREE", "ref", [](const pth::Tuning& x) { return (long long)x.bvh_tree_ref; }, 1},
        {"PT_BVH_TREE", "sah", [](const pth::Tuning& x) { return (long long)x.bvh_tree_ref; }, 0},
        {"PT_TAIL", "0", [](const pth::Tuning& x) { return (long long)x.tail_off; }, 1},
        {"PT_TAIL", "1", [](const pth::Tuning& x) { return (long long)x.tail_off; }, 0},
        {"PT_BOUNCE_LDS_PAD", "-4", [](const pth::Tuning& x) { return (long long)x.bounce_lds_pad; }, 0},
        {"PT_BVH_TAIL_TRAV_BLOCKS", "0", [](const pth::Tuning& x) { return (long long)x.tail_trav_blocks; }, 1},
        {"PT_BVH_QUAD", "5", [](const pth::Tuning& x) { return (long long)x.bvh_quad; }, 1},
        {"PT_SPECULATE", "0", [](const pth::Tuning& x) { return (long long)x.speculate; }, 0},
        {"PT_SPECULATE", "", [](const pth::Tuning& x) { return (long long)x.speculate; }, 1},   // empty: the default
    };
    for (const Case& c : cases) {
        setenv(c.name, c.value, 1);
        const long long got = c.get(pth::read_tuning());
        unsetenv(c.name);
        CHECK(got == c.want, "%s=%s gives %lld, expected %lld", c.name, c.value, got, c.want);
    }
    printf("tuning ok cases=%zu\n", sizeof cases / sizeof cases[0]);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string part = argc > 1 ? argv[1] : "";
    if (part != "" && part != "bands" && part != "worker" && part != "tuning") {
        fprintf(stderr, "usage: %s [bands|worker|tuning]\n", argv[0]);
        return 2;
    }
    if (part == "" || part == "bands") check_bands();
    if (!g_failed && (part == "" || part == "worker")) check_worker();
    if (!g_failed && (part == "" || part == "tuning")) check_tuning();
    return g_failed;
}
