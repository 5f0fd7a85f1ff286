/*
 * policy_ms_cp.cpp -- urf_policy::multi_sector_cp (urf_set_front_multi_sector_curb_points) in urf_policy::plan and urf_front_family_of
 * (urban_road_filter_amd/csrc/urf_policy.hpp), without HIP and without a GPU:   g++ -std=c++17 -O2 -I include -I urban_road_filter_amd/csrc
 *
 * Walks front mode x channels x curbPoints 1..9 x star-shaped search x multi_sector x curb_points x lasers128 x slot / batch x a small and a
 * large n_scans (x the row-major states that let a slot or a small batch take the fused kernels) and checks, row by row:
 *   (1) multi_sector_cp off: front_ms is the rule from before the switch -- front && multi_sector && star && curbPoints == 5;
 *   (2) off against on: nothing plan() writes differs except front_ms (the whole urf_kargs is compared, front_ms put aside);
 *   (3) on: front_ms == front && multi_sector && star && 1 <= curbPoints <= 8;
 *   (4) either way: urf_front_family_of(...).ms == front_ms, and .cp == curbPoints for a fused call with curbPoints 1..8.
 * Prints "rows N fused F ms_off A ms_on B" and returns 0, or the first row that fails and 1.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "urf_policy.hpp"

namespace {

struct Row {
    int mode, channels, cp, star, multi_sector, curb_points, lasers128, slot, rows_state;
    uint32_t n_scans;
};

int fail(const Row& r, const char* what, unsigned got, unsigned want)
{
    printf("FAILED %s: got %u, want %u at front_mode %d channels %d curbPoints %d star %d multi_sector %d curb_points %d lasers128 %d slot %d "
           "rows_state %d n_scans %u\n",
           what, got, want, r.mode, r.channels, r.cp, r.star, r.multi_sector, r.curb_points, r.lasers128, r.slot, r.rows_state, r.n_scans);
    return 1;
}

urf_kargs plan_of(const Row& r, bool multi_sector_cp, const urf_dev_params& dp)
{
    urf_policy p;
    p.front_mode = r.mode;
    p.lasers128 = r.lasers128 != 0, p.curb_points = r.curb_points != 0, p.multi_sector = r.multi_sector != 0;
    p.multi_sector_cp = multi_sector_cp;
    /* rows_state: 0 never sighted, 1 sighted and used (a slot, a small batch of mode 1 take the fused kernels) */
    p.front_rows = r.rows_state == 1, p.rows_used = r.rows_state == 1;
    urf_kargs a;
    memset(&a, 0, sizeof a);
    a.tiles = 4u, a.n_scans = r.n_scans, a.capture = 0u;
    p.plan(a, dp, r.slot != 0, false);
    return a;
}

}   // namespace

int main()
{
    static const int CHANNELS[] = { 16, 32, 64, 128 };
    static const uint32_t N_SCANS[] = { 4u, 1024u };
    unsigned long long rows = 0, fused = 0, ms_off = 0, ms_on = 0;
    urf_dev_params dp;
    memset(&dp, 0, sizeof dp);
    for (int mode = 0; mode <= 3; mode++)
    for (int channels : CHANNELS)
    for (int cp = 1; cp <= 9; cp++)
    for (int star = 0; star <= 1; star++)
    for (int multi_sector = 0; multi_sector <= 1; multi_sector++)
    for (int curb_points = 0; curb_points <= 1; curb_points++)
    for (int lasers128 = 0; lasers128 <= 1; lasers128++)
    for (int slot = 0; slot <= 1; slot++)
    for (int rows_state = 0; rows_state <= 1; rows_state++)
    for (uint32_t n_scans : N_SCANS) {
        const Row r = { mode, channels, cp, star, multi_sector, curb_points, lasers128, slot, rows_state, n_scans };
        dp.p.channels = channels, dp.p.curbPoints = cp, dp.p.star_shaped_method = star;
        urf_kargs off = plan_of(r, false, dp), on = plan_of(r, true, dp);
        const bool front = off.front != 0u;
        /* (1) */
        const unsigned today = (front && multi_sector && star && cp == 5) ? 1u : 0u;
        if (off.front_ms != today)
            return fail(r, "front_ms with the switch off", off.front_ms, today);
        /* (3) */
        const unsigned want = (on.front != 0u && multi_sector && star && cp >= 1 && cp <= 8) ? 1u : 0u;
        if (on.front_ms != want)
            return fail(r, "front_ms with the switch on", on.front_ms, want);
        /* (4) */
        for (const urf_kargs* a : { &off, &on }) {
            const urf_front_family f = urf_front_family_of(a->front, a->front_lsh, a->front_rows, a->front_ms, a->tiles, cp);
            if (f.ms != a->front_ms)
                return fail(r, "family.ms", f.ms, a->front_ms);
            if (f.fused != a->front)
                return fail(r, "family.fused", f.fused, a->front);
            if (a->front && cp <= 8 && f.cp != cp)
                return fail(r, "family.cp", f.cp, (unsigned)cp);
        }
        if (front && cp == 9)
            return fail(r, "front at curbPoints 9", 1u, 0u);
        rows++, fused += front, ms_off += off.front_ms, ms_on += on.front_ms;
        /* (2) */
        off.front_ms = on.front_ms = 0u;
        if (memcmp(&off, &on, sizeof off) != 0)
            return fail(r, "a field besides front_ms differs between the switch off and on (front)", on.front, off.front);
    }
    printf("rows %llu fused %llu ms_off %llu ms_on %llu\n", rows, fused, ms_off, ms_on);
    return 0;
}
