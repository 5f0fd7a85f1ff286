/*
 * policy_auto.cpp -- urf_set_front_auto's two pure functions, urf_policy::auto_call and urf_policy::auto_digest
 * (urban_road_filter_amd/csrc/urf_policy.hpp), without HIP and without a GPU:   g++ -std=c++17 -O2 -pthread -I include -I urban_road_filter_amd/csrc
 *
 * The walk is policy_why.cpp's cross product of settings and calls, less front_direct, front_tpb and front_outputs (neither why() nor
 * a.front reads the first two, the third only decides the FRONT_OUTPUTS bit, which auto never applies).  On every row:
 *   (a) plan() decides the same with the auto fields at their defaults and with every one of them set: it reads none of them;
 *   (b) front modes 0 and 1, or the switch off: auto_call applies nothing;
 *   (c) front modes 2 and 3, the switch on: the bits lie inside URF_ADVICE_AUTO_MASK; applied (switches on, mode 3), auto_call of the
 *       re-asked why() is empty -- a fixed point in one step --, and the call is fused exactly where the original advice held no bit
 *       outside URF_ADVICE_AUTO_MASK | MODE_2;
 *   (d) a refused bit is not asked for again, and the call then stays with the general kernels.
 * Then auto_digest over a hand-written table of digests (digests()).
 *   policy_auto     prints "rows N applied K fused F failures 0" and returns 0, or the first failing rows and 1
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "urf_policy.hpp"

namespace {

struct Var {
    const char* name;
    int n;
    int values[8];
};
enum { FRONT_MODE, CHANNELS, LASERS128, CURB_POINTS, MULTI_SECTOR, MULTI_SECTOR_CP, LONG_SWEEPS, WANT_RING_SORTED, FRONT_OFF, ROWS_STATE, CP, STAR, TILES,
       N_SCANS, CAPTURE, SLOT, GENERAL_ONLY, N_IN };
const Var IN[N_IN] = {
    { "front_mode", 4, { 0, 1, 2, 3 } },
    { "channels", 5, { 8, 16, 32, 64, 128 } },
    { "lasers128", 2, { 0, 1 } },
    { "curb_points", 2, { 0, 1 } },
    { "multi_sector", 2, { 0, 1 } },
    { "multi_sector_cp", 2, { 0, 1 } },
    { "long_sweeps", 2, { 0, 1 } },
    { "want_ring_sorted", 2, { 0, 1 } },
    { "front_off", 2, { 0, 1 } },
    { "rows_state", 5, { 0, 1, 2, 3, 4 } },
    { "curbPoints", 5, { 1, 4, 5, 8, 9 } },
    { "star_shaped_method", 2, { 0, 1 } },
    { "tiles", 6, { 1, 2, 128, 129, 256, 257 } },
    { "n_scans", 7, { 1, 15, 16, 191, 192, 511, 512 } },
    { "capture", 2, { 0, 1 } },
    { "slot", 2, { 0, 1 } },
    { "general_only", 2, { 0, 1 } },
};

thread_local uint32_t g_flags[URF_FLAG_WORDS];
thread_local urf_kargs g_a;
thread_local urf_dev_params g_dp;

struct Row {
    urf_policy p;
    uint32_t tiles, n_scans, capture;
    bool slot, general_only;
};

void make(const int* v, Row& r)
{
    r.p = urf_policy();
    r.p.flags = g_flags;
    r.p.front_mode = v[FRONT_MODE];
    r.p.lasers128 = v[LASERS128], r.p.curb_points = v[CURB_POINTS], r.p.multi_sector = v[MULTI_SECTOR], r.p.multi_sector_cp = v[MULTI_SECTOR_CP];
    r.p.long_sweeps = v[LONG_SWEEPS], r.p.want_ring_sorted = v[WANT_RING_SORTED], r.p.front_off = v[FRONT_OFF];
    const int rs = v[ROWS_STATE];
    r.p.front_rows = rs >= 1 && rs <= 3, r.p.rows_used = rs == 2, r.p.rows_probation = rs == 1 ? 16u : 0u, r.p.rows_oom = rs == 4;
    g_dp.p.channels = v[CHANNELS], g_dp.p.curbPoints = v[CP], g_dp.p.star_shaped_method = v[STAR];
    r.tiles = (uint32_t)v[TILES], r.n_scans = (uint32_t)v[N_SCANS], r.capture = (uint32_t)v[CAPTURE];
    r.slot = v[SLOT] != 0, r.general_only = v[GENERAL_ONLY] != 0;
}

/* everything plan() writes, in one comparable record */
struct Plan {
    uint32_t w[10];
    bool operator==(const Plan& o) const { return memcmp(w, o.w, sizeof w) == 0; }
};
Plan plan_of(const Row& r)
{
    g_a.tiles = r.tiles, g_a.n_scans = r.n_scans, g_a.capture = r.capture;
    r.p.plan(g_a, g_dp, r.slot, r.general_only);
    return Plan{ { g_a.front, g_a.front_sight, g_a.front_tpb, g_a.front_lists, g_a.front_rows, g_a.front_ms, g_a.front_lsh, g_a.table_lookahead, g_a.table_hint,
                   g_a.optimistic } };
}
urf_policy::reasons why_of(const Row& r)
{
    g_a.tiles = r.tiles, g_a.n_scans = r.n_scans, g_a.capture = r.capture;
    return r.p.why(g_a, g_dp, r.slot, r.general_only);
}

/* what urf_api.hip's auto_apply does to the policy: the switches on, mode 3 */
void apply(urf_policy& p, uint32_t bits)
{
    if (bits & URF_ADVICE_MODE_3)
        p.front_mode = 3;
    if (bits & URF_ADVICE_LASERS128)
        p.lasers128 = true;
    if (bits & URF_ADVICE_LONG_SWEEPS)
        p.long_sweeps = true;
    if (bits & URF_ADVICE_CURB_POINTS)
        p.curb_points = true;
    if (bits & URF_ADVICE_MULTI_SECTOR)
        p.multi_sector = true;
    if (bits & URF_ADVICE_MULTI_SECTOR_CP)
        p.multi_sector_cp = true;
    p.auto_applied |= bits;
}

bool next(int first, int* idx, int* v)
{
    for (int k = N_IN - 1; k >= first; k--) {
        if (++idx[k] == IN[k].n)
            idx[k] = 0;
        v[k] = IN[k].values[idx[k]];
        if (idx[k])
            return true;
    }
    return false;
}

struct Tally {
    unsigned long long rows = 0, applied = 0, fused = 0, failures = 0;
};
std::mutex g_print;
std::atomic<unsigned long long> g_printed{ 0 };

void slice(int mode, int channels, Tally& sum)
{
    int idx[N_IN] = { 0 }, v[N_IN];
    for (int k = 0; k < N_IN; k++)
        v[k] = IN[k].values[0];
    v[FRONT_MODE] = mode, v[CHANNELS] = channels;
    Row r;
    auto fail = [&](const char* what, uint32_t why, uint32_t adv) {
        sum.failures++;
        if (g_printed++ < 20) {
            std::lock_guard<std::mutex> lock(g_print);
            printf("FAIL %s why=%#x advice=%#x:", what, why, adv);
            for (int k = 0; k < N_IN; k++)
                printf(" %s=%d", IN[k].name, v[k]);
            printf("\n");
        }
    };
    do {
        make(v, r);
        sum.rows++;
        const Plan off = plan_of(r);
        const urf_policy::reasons y = why_of(r);
        if (r.p.auto_call(y.why, y.advice) != 0u)
            fail("(b) the switch is off", y.why, y.advice);
        Row t = r;
        t.p.auto_on = true, t.p.auto_phase = URF_AUTO_LEARNING, t.p.auto_applied = URF_ADVICE_AUTO_MASK, t.p.auto_again = 2, t.p.auto_explained = 4;
        t.p.auto_wait = 1, t.p.auto_seq = 7, t.p.auto_left = t.p.auto_left_digest = URF_ADVICE_NEVER;
        if (!(plan_of(t) == off))
            fail("(a) plan() reads an auto field", y.why, y.advice);
        t.p.auto_applied = 0;
        const uint32_t bits = t.p.auto_call(y.why, y.advice);
        if (mode < 2) {
            if (bits)
                fail("(b) front modes 0 and 1", y.why, bits);
            continue;
        }
        if (bits & ~URF_ADVICE_AUTO_MASK)
            fail("(c) a bit outside the mask", y.why, bits);
        if ((y.advice & (URF_ADVICE_NEVER | URF_ADVICE_CAPTURE_OFF | URF_ADVICE_RESET)) && bits)
            fail("(c) applied next to NEVER / CAPTURE_OFF / RESET", y.why, bits);
        Row d = t;   /* (d): the first bit refused */
        apply(t.p, bits);
        sum.applied += bits != 0u;
        const urf_policy::reasons z = why_of(t);
        if (t.p.auto_call(z.why, z.advice) != 0u)
            fail("(c) no fixed point in one step", z.why, z.advice);
        const bool fused = plan_of(t).w[0] != 0u;
        sum.fused += fused;
        if (fused != ((y.advice & ~(URF_ADVICE_AUTO_MASK | URF_ADVICE_MODE_2)) == 0u))
            fail("(c) fused <=> the advice lay inside the mask", y.why, y.advice);
        if (bits) {
            d.p.auto_refused = bits & (0u - bits);
            const uint32_t rest = d.p.auto_call(y.why, y.advice);
            if (rest != (bits & ~d.p.auto_refused))
                fail("(d) a refused bit is asked for again", y.why, rest);
            apply(d.p, rest);
            if (plan_of(d).w[0] != 0u)
                fail("(d) fused without a bit the advice needs (why()'s advice is minimal)", y.why, rest);
        }
    } while (next(CHANNELS + 1, idx, v));
}

/* ---- auto_digest: seq, scans, handed_back, scan_bits, helped, never, candidates, other ---- */
int digests()
{
    int failures = 0;
    auto check = [&](const char* what, bool ok) {
        if (!ok) {
            printf("FAIL digest: %s\n", what);
            failures++;
        }
    };
    const uint32_t MS = URF_WHY_SCAN_MULTI_SECTOR, FALL = URF_WHY_SCAN_SECTORS_FALL, SHAPE = URF_WHY_SCAN_LANE_TWO_RINGS | URF_WHY_SCAN_AXIS;
    urf_dev_params dp;
    memset(&dp, 0, sizeof dp);
    dp.p.channels = 64, dp.p.star_shaped_method = 1;
    for (int cp : { 5, 3 }) {
        dp.p.curbPoints = cp;
        const uint32_t want = URF_ADVICE_MULTI_SECTOR | (cp != 5 ? URF_ADVICE_MULTI_SECTOR_CP : 0u);
        urf_policy p;
        p.front_mode = cp == 5 ? 2 : 3, p.auto_on = true, p.auto_phase = URF_AUTO_LEARNING;
        const uint32_t helped[8] = { 1, 4, 3, MS | FALL | SHAPE, 2, 1, 0, 0 };   /* two scans the switch keeps, one nothing helps */
        urf_policy::auto_step s = p.auto_digest(helped, dp);
        check("MULTI_SECTOR (and _CP off curbPoints 5) is applied, still learning", s.apply == want && s.phase == URF_AUTO_LEARNING && !s.again);
        apply(p, s.apply);
        s = p.auto_digest(helped, dp);   /* ... once: with the switches on the same digest asks for nothing (and cannot come again) */
        check("... once", s.apply == 0u);
        const uint32_t after[8] = { 2, 4, 1, SHAPE, 0, 1, 0, 0 };
        s = p.auto_digest(after, dp);
        check("all never: settled", s.apply == 0u && s.phase == URF_AUTO_SETTLED);
        urf_policy q;
        q.front_mode = 2, q.auto_on = true, q.auto_phase = URF_AUTO_LEARNING, q.auto_refused = want;
        s = q.auto_digest(helped, dp);
        check("refused: not applied again", s.apply == 0u);
        if (cp != 5) {   /* multi_sector on by hand, _CP missing */
            urf_policy h;
            h.front_mode = 3, h.auto_on = true, h.auto_phase = URF_AUTO_LEARNING, h.multi_sector = true;
            s = h.auto_digest(helped, dp);
            check("only _CP is missing", s.apply == URF_ADVICE_MULTI_SECTOR_CP);
        }
    }
    dp.p.curbPoints = 5;
    urf_policy p;
    p.front_mode = 2, p.auto_on = true, p.auto_phase = URF_AUTO_LEARNING;
    const uint32_t clean[8] = { 3, 4, 0, 0, 0, 0, 0, 0 };
    urf_policy::auto_step s = p.auto_digest(clean, dp);
    check("clean: settled", s.apply == 0u && s.phase == URF_AUTO_SETTLED && !s.again);
    const uint32_t never_cand[8] = { 4, 8, 3, SHAPE | URF_WHY_SCAN_CANDIDATES, 0, 2, 1, 0 };
    s = p.auto_digest(never_cand, dp);
    check("never + candidates == handed back: settled", s.apply == 0u && s.phase == URF_AUTO_SETTLED);
    const uint32_t other[8] = { 5, 4, 2, URF_WHY_SCAN_OTHER | SHAPE, 0, 1, 0, 1 };
    for (int k = 0; k < 4; k++) {
        s = p.auto_digest(other, dp);
        check("OTHER three times, settled on the fourth", s.apply == 0u && (k < 3 ? (s.phase == URF_AUTO_LEARNING && s.again) : (s.phase == URF_AUTO_SETTLED && !s.again)));
        if (s.again)
            p.auto_again++;
    }
    p.auto_again = 0;
    const uint32_t sighting[8] = { 6, 1, 1, URF_WHY_SCAN_ROWS_SIGHTING, 0, 0, 0, 0 };
    s = p.auto_digest(sighting, dp);
    check("a first sighting: again", s.phase == URF_AUTO_LEARNING && s.again);
    /* never a bit outside the mask, whatever the words */
    for (uint32_t k = 0; k < 4096u; k++) {
        const uint32_t d[8] = { k, k & 7u, (k >> 3) & 7u, (k * 37u) & 0x3ffu, (k >> 6) & 3u, (k >> 8) & 3u, (k >> 10) & 1u, (k >> 11) & 1u };
        for (int cp : { 5, 8 })
            for (int mode = 0; mode < 4; mode++) {
                urf_policy z;
                z.front_mode = mode, z.auto_on = true, z.auto_phase = URF_AUTO_LEARNING, z.multi_sector = (k & 1u) != 0u;
                dp.p.curbPoints = cp;
                s = z.auto_digest(d, dp);
                check("bits inside the mask, phases by name, nothing below mode 2",
                      (s.apply & ~URF_ADVICE_AUTO_MASK) == 0u && s.phase <= URF_AUTO_SETTLED && (mode >= 2 || (s.apply == 0u && s.phase == URF_AUTO_IDLE)));
            }
    }
    return failures;
}

}   // namespace

int main()
{
    const int n_slices = IN[FRONT_MODE].n * IN[CHANNELS].n;
    unsigned n_threads = std::thread::hardware_concurrency();
    n_threads = n_threads < 1u ? 1u : (n_threads > 16u ? 16u : n_threads);
    std::vector<Tally> sums(n_threads);
    std::atomic<int> at{ 0 };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < n_threads; t++)
        pool.emplace_back([&, t]() {
            for (int k; (k = at++) < n_slices;)
                slice(IN[FRONT_MODE].values[k / IN[CHANNELS].n], IN[CHANNELS].values[k % IN[CHANNELS].n], sums[t]);
        });
    Tally all;
    for (unsigned t = 0; t < n_threads; t++) {
        pool[t].join();
        all.rows += sums[t].rows, all.applied += sums[t].applied, all.fused += sums[t].fused, all.failures += sums[t].failures;
    }
    all.failures += (unsigned long long)digests();
    printf("rows %llu applied %llu fused %llu failures %llu\n", all.rows, all.applied, all.fused, all.failures);
    return all.failures ? 1 : 0;
}
