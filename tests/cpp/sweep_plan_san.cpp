// The removals-only form of the mirror host plan (opendht_amd/csrc/kad_mirror_plan.cpp: strictly ascending
// KAD_OP_REMOVE rows, what kad_table_expire hands it) against the general form of the same plan (the same rows with
// the first and last swapped, which takes the map-based path): every field of the two plans must be equal, over
// random directories with empty buckets, sparse, dense and total removals; a duplicate and an out-of-range node are
// still refused. mirror_plan_removals (the plain node list of kad_table_expire) is held to the same plans. Built with -fsanitize=address,undefined by tests/test_sweep_plan_san.py. CPU only. Exit 0 = pass.
#include "../../opendht_amd/csrc/kad_mirror_plan.h"
#include "kadgpu.h"
#include <cstdio>
#include <random>
#include <algorithm>
using namespace kadplan;
int main() {
    std::mt19937 g(5);
    int bad = 0;
    for (int it = 0; it < 300; it++) {
        uint32_t B = 1 + g() % 60;
        std::vector<uint32_t> off(B + 1, 0);
        for (uint32_t b = 0; b < B; b++) off[b + 1] = off[b] + (g() % 4 == 0 ? 0 : g() % 12);
        uint32_t n = off[B];
        std::vector<uint8_t> first(20 * B, 0);
        for (uint32_t b = 0; b < B; b++) { first[20 * b] = b >> 8; first[20 * b + 1] = b; }
        std::vector<uint32_t> rm;
        int mode = it % 3;
        for (uint32_t i = 0; i < n; i++) if (mode == 2 || g() % (mode ? 2 : 9) == 0) rm.push_back(i);
        if (rm.empty()) continue;
        std::vector<uint32_t> a(3 * rm.size()), b2;
        for (size_t k = 0; k < rm.size(); k++) { a[3 * k] = KAD_OP_REMOVE; a[3 * k + 1] = rm[k]; a[3 * k + 2] = 0; }
        std::vector<uint32_t> sh = rm;
        if (sh.size() > 1) std::swap(sh[0], sh[sh.size() - 1]); else { continue; }
        b2.resize(3 * sh.size());
        for (size_t k = 0; k < sh.size(); k++) { b2[3 * k] = KAD_OP_REMOVE; b2[3 * k + 1] = sh[k]; b2[3 * k + 2] = 0; }
        MirrorPlan p1, p2; std::string e;
        OldIds none = [](uint32_t, uint32_t, uint8_t*) { return 0; };
        int r1 = mirror_plan(off, first.data(), n, a.data(), rm.size(), nullptr, 0, -1, 0, none, p1, e);
        int r2 = mirror_plan(off, first.data(), n, b2.data(), sh.size(), nullptr, 0, -1, 0, none, p2, e);
        bool same = r1 == 0 && r2 == 0 && p1.B1 == p2.B1 && p1.n1 == p2.n1 && p1.off1 == p2.off1 && p1.list == p2.list &&
                    p1.first1 == p2.first1 && p1.segs.size() == p2.segs.size() && p1.new_in_range == p2.new_in_range;
        for (size_t s = 0; same && s < p1.segs.size(); s++)
            same = p1.segs[s].start == p2.segs[s].start && p1.segs[s].src == p2.segs[s].src && p1.segs[s].len == p2.segs[s].len && p1.segs[s].kind == p2.segs[s].kind;
        // the list form kad_table_expire hands over (node indices plus a base) gives the same plan again
        const uint32_t base = it % 2 ? 0x7FFF0000u : 0u;
        std::vector<uint32_t> lst(rm);
        for (auto& x : lst) x += base;
        MirrorPlan p3;
        int r3 = mirror_plan_removals(off, n, lst.data(), (uint32_t)lst.size(), base, p3, e);
        same = same && r3 == 0 && p3.B1 == p1.B1 && p3.n1 == p1.n1 && p3.off1 == p1.off1 && p3.list == p1.list &&
               p3.segs.size() == p1.segs.size() && p3.first1.empty();
        for (size_t s = 0; same && s < p1.segs.size(); s++)
            same = p1.segs[s].start == p3.segs[s].start && p1.segs[s].src == p3.segs[s].src && p1.segs[s].len == p3.segs[s].len && p1.segs[s].kind == p3.segs[s].kind;
        if (!same) { bad++; std::printf("mismatch it=%d r=%d %d segs %zu %zu\n", it, r1, r2, p1.segs.size(), p2.segs.size()); }
    }
    // a duplicate and an out-of-range node are refused as before
    std::vector<uint32_t> off = {0, 3}; std::vector<uint8_t> first(20, 0);
    uint32_t dup[6] = {1, 1, 0, 1, 1, 0}, oor[3] = {1, 3, 0};
    MirrorPlan p; std::string e; OldIds none = [](uint32_t, uint32_t, uint8_t*) { return 0; };
    if (mirror_plan(off, first.data(), 3, dup, 2, nullptr, 0, -1, 0, none, p, e) == 0) { bad++; std::printf("dup accepted\n"); }
    if (mirror_plan(off, first.data(), 3, oor, 1, nullptr, 0, -1, 0, none, p, e) == 0) { bad++; std::printf("oor accepted\n"); }
    uint32_t l_dup[2] = {1, 1}, l_oor[1] = {3}, l_desc[2] = {2, 1}, l_low[1] = {4};
    if (mirror_plan_removals(off, 3, l_dup, 2, 0, p, e) == 0) { bad++; std::printf("list dup accepted\n"); }
    if (mirror_plan_removals(off, 3, l_oor, 1, 0, p, e) == 0) { bad++; std::printf("list oor accepted\n"); }
    if (mirror_plan_removals(off, 3, l_desc, 2, 0, p, e) == 0) { bad++; std::printf("list descending accepted\n"); }
    if (mirror_plan_removals(off, 3, l_low, 1, 5, p, e) == 0) { bad++; std::printf("list below base accepted\n"); }
    std::printf(bad ? "FAIL %d\n" : "PASS\n", bad);
    return bad != 0;
}
