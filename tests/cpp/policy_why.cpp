/*
 * policy_why.cpp -- urf_policy::why (urban_road_filter_amd/csrc/urf_policy.hpp) against urf_policy::plan over the cross product of
 * policy_table.cpp's inputs plus multi_sector_cp, without HIP and without a GPU:   g++ -std=c++17 -O2 -I include -I urban_road_filter_amd/csrc
 *
 * On every row:
 *   (a) why == 0 if and only if plan() gives front == 1;
 *   (b) without NEVER: the advice applied to a copy of the policy and the call -- the mode raised to the advised one, the advised switches
 *       on, RESET = forget_front() + want_ring_sorted = false (and the call is no read-out's own run: general_only = false), CAPTURE_OFF,
 *       BATCH = slot = false with n_scans = 512 -- gives front == 1 and why == 0;
 *   (c) minimal: the advice without any single bit leaves front == 0.  FRONT_OUTPUTS is the one bit plan() does not read (it keeps the next
 *       read-out from turning the context general again, RESET undoes the last one): it must come with READOUT exactly when the switch is
 *       off, and is left out of the advice that (b) and (c) apply;
 *   (d) with NEVER: no assignment of mode and switches gives front == 1 for the row's channels / curbPoints / tiles, with everything else
 *       in the call's favour.
 *   policy_why                    prints "rows N front F never K failures 0" and returns 0, or the first failing rows and 1
 *   policy_why name=value ...     one row, the inputs not named at their first value: "front why advice"
 * The (front_mode, channels) slices are walked by up to 16 threads (-pthread).
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "urf_policy.hpp"

namespace {

struct Var {
    const char* name;
    int n;
    int values[8];
};
enum { FRONT_MODE, CHANNELS, LASERS128, CURB_POINTS, MULTI_SECTOR, MULTI_SECTOR_CP, LONG_SWEEPS, WANT_RING_SORTED, FRONT_OUTPUTS, FRONT_OFF, FRONT_DIRECT,
       FRONT_TPB, ROWS_STATE, CP, STAR, TILES, N_SCANS, CAPTURE, SLOT, GENERAL_ONLY, N_IN };
/* policy_table.cpp's values; multi_sector_cp and front_outputs (which why() reads) added */
const Var IN[N_IN] = {
    { "front_mode", 4, { 0, 1, 2, 3 } },
    { "channels", 5, { 8, 16, 32, 64, 128 } },
    { "lasers128", 2, { 0, 1 } },
    { "curb_points", 2, { 0, 1 } },
    { "multi_sector", 2, { 0, 1 } },
    { "multi_sector_cp", 2, { 0, 1 } },
    { "long_sweeps", 2, { 0, 1 } },
    { "want_ring_sorted", 2, { 0, 1 } },
    { "front_outputs", 2, { 0, 1 } },
    { "front_off", 2, { 0, 1 } },
    { "front_direct", 2, { 0, 1 } },
    { "front_tpb", 3, { 0, 1, 3 } },
    { "rows_state", 5, { 0, 1, 2, 3, 4 } },
    { "curbPoints", 5, { 1, 4, 5, 8, 9 } },
    { "star_shaped_method", 2, { 0, 1 } },
    { "tiles", 6, { 1, 2, 128, 129, 256, 257 } },
    { "n_scans", 7, { 1, 15, 16, 191, 192, 511, 512 } },
    { "capture", 2, { 0, 1 } },
    { "slot", 2, { 0, 1 } },
    { "general_only", 2, { 0, 1 } },
};

thread_local uint32_t g_flags[URF_FLAG_WORDS];   /* (forget_front writes them: a thread's own, like everything a row touches) */

/* a row: the policy and what plan() reads of the call (the parameters: g_dp, the row's) */
struct Row {
    urf_policy p;
    uint32_t tiles, n_scans, capture;
    bool slot, general_only;
};
thread_local urf_kargs g_a;   /* (zero: plan() writes what it decides) */
thread_local urf_dev_params g_dp;

void make(const int* v, Row& r)
{
    r.p = urf_policy();
    r.p.flags = g_flags;
    r.p.front_mode = v[FRONT_MODE];
    r.p.lasers128 = v[LASERS128], r.p.curb_points = v[CURB_POINTS], r.p.multi_sector = v[MULTI_SECTOR], r.p.multi_sector_cp = v[MULTI_SECTOR_CP];
    r.p.long_sweeps = v[LONG_SWEEPS], r.p.want_ring_sorted = v[WANT_RING_SORTED], r.p.front_outputs = v[FRONT_OUTPUTS];
    r.p.front_off = v[FRONT_OFF], r.p.front_direct = v[FRONT_DIRECT], r.p.front_tpb = (uint32_t)v[FRONT_TPB];
    const int rs = v[ROWS_STATE];
    r.p.front_rows = rs >= 1 && rs <= 3, r.p.rows_used = rs == 2, r.p.rows_probation = rs == 1 ? 16u : 0u, r.p.rows_oom = rs == 4;
    g_dp.p.channels = v[CHANNELS], g_dp.p.curbPoints = v[CP], g_dp.p.star_shaped_method = v[STAR];
    r.tiles = (uint32_t)v[TILES], r.n_scans = (uint32_t)v[N_SCANS], r.capture = (uint32_t)v[CAPTURE];
    r.slot = v[SLOT] != 0, r.general_only = v[GENERAL_ONLY] != 0;
}

bool front_of(const Row& r)
{
    g_a.tiles = r.tiles, g_a.n_scans = r.n_scans, g_a.capture = r.capture;
    r.p.plan(g_a, g_dp, r.slot, r.general_only);
    return g_a.front != 0u;
}
urf_policy::reasons why_of(const Row& r)
{
    g_a.tiles = r.tiles, g_a.n_scans = r.n_scans, g_a.capture = r.capture;
    return r.p.why(g_a, g_dp, r.slot, r.general_only);
}

/* the row with the advice applied */
void apply(Row& r, uint32_t adv)
{
    if ((adv & URF_ADVICE_MODE_3) && r.p.front_mode < 3)
        r.p.front_mode = 3;
    if ((adv & URF_ADVICE_MODE_2) && r.p.front_mode < 2)
        r.p.front_mode = 2;
    if (adv & URF_ADVICE_LASERS128)
        r.p.lasers128 = true;
    if (adv & URF_ADVICE_LONG_SWEEPS)
        r.p.long_sweeps = true;
    if (adv & URF_ADVICE_CURB_POINTS)
        r.p.curb_points = true;
    if (adv & URF_ADVICE_MULTI_SECTOR)
        r.p.multi_sector = true;
    if (adv & URF_ADVICE_MULTI_SECTOR_CP)
        r.p.multi_sector_cp = true;
    if (adv & URF_ADVICE_FRONT_OUTPUTS)
        r.p.front_outputs = true;
    if (adv & URF_ADVICE_RESET) {
        r.p.forget_front();
        r.p.want_ring_sorted = false;
        r.general_only = false;
    }
    if (adv & URF_ADVICE_CAPTURE_OFF)
        r.capture = 0;
    if (adv & URF_ADVICE_BATCH) {
        r.slot = false;
        r.n_scans = 512;
    }
}

/* (d): does ANY mode and any switches fuse these channels / curbPoints / tiles (a large batch call, nothing else in its way) */
bool possible(int channels, int cp, int tiles)
{
    thread_local int8_t memo[256][32][512];
    int8_t& m = memo[channels & 255][cp & 31][tiles & 511];
    if (m)
        return m > 0;
    bool any = false;
    for (int mode = 0; mode < 4; mode++)
        for (int sw = 0; sw < 64; sw++) {
            Row r;
            r.p = urf_policy();
            r.p.flags = g_flags;
            r.p.front_mode = mode;
            r.p.lasers128 = sw & 1, r.p.long_sweeps = sw & 2, r.p.curb_points = sw & 4, r.p.multi_sector = sw & 8, r.p.multi_sector_cp = sw & 16, r.p.front_outputs = sw & 32;
            const urf_dev_params row_dp = g_dp;
            g_dp.p.channels = channels, g_dp.p.curbPoints = cp, g_dp.p.star_shaped_method = 1;
            r.tiles = (uint32_t)tiles, r.n_scans = 512, r.capture = 0;
            r.slot = r.general_only = false;
            any = any || front_of(r);
            g_dp = row_dp;
        }
    m = any ? 1 : -1;
    return any;
}

/* the next combination of the variables from `first` on, the last one fastest; false after the last */
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
    unsigned long long rows = 0, fronts = 0, nevers = 0, failures = 0;
};
std::mutex g_print;
std::atomic<unsigned long long> g_printed{ 0 };

/* the rows of one front_mode and one channels */
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
        const bool front = front_of(r);
        const urf_policy::reasons y = why_of(r);
        sum.fronts += front;
        if ((y.why == 0u) != front)
            fail("(a) why == 0 <=> front", y.why, y.advice);
        if (front) {
            if (y.advice)
                fail("advice for a fused call", y.why, y.advice);
            continue;
        }
        const bool readout = (y.why & URF_WHY_CALL_READOUT) != 0u;
        if (((y.advice & URF_ADVICE_FRONT_OUTPUTS) != 0u) != (readout && !r.p.front_outputs) || (readout && !(y.advice & URF_ADVICE_RESET)))
            fail("(c) FRONT_OUTPUTS goes with READOUT while the switch is off, RESET with it", y.why, y.advice);
        const uint32_t adv = y.advice & ~URF_ADVICE_FRONT_OUTPUTS;
        if (adv & URF_ADVICE_NEVER) {
            sum.nevers++;
            if (possible(v[CHANNELS], v[CP], v[TILES]))
                fail("(d) NEVER, but some settings fuse it", y.why, y.advice);
            continue;
        }
        if (!possible(v[CHANNELS], v[CP], v[TILES]))
            fail("(d) no settings fuse it, but no NEVER", y.why, y.advice);
        Row t = r;
        apply(t, adv);
        if (!front_of(t) || why_of(t).why != 0u)
            fail("(b) the advice applied", y.why, y.advice);
        if (adv == 0u)
            fail("(b) no advice", y.why, y.advice);
        for (uint32_t bit = 1u; bit <= adv; bit <<= 1) {
            if (!(adv & bit))
                continue;
            Row d = r;
            apply(d, adv & ~bit);
            if (front_of(d))
                fail("(c) not minimal", y.why, bit);
        }
    } while (next(CHANNELS + 1, idx, v));
}

}   // namespace

int main(int argc, char** argv)
{
    if (argc > 1) {   /* policy_why name=value ...: one row (the other inputs at their first value), "front why advice" */
        int v[N_IN];
        for (int k = 0; k < N_IN; k++)
            v[k] = IN[k].values[0];
        for (int i = 1; i < argc; i++) {
            const char* eq = strchr(argv[i], '=');
            int k = 0;
            while (eq && k < N_IN && std::string(argv[i], (size_t)(eq - argv[i])) != IN[k].name)
                k++;
            if (!eq || k == N_IN) {
                fprintf(stderr, "usage: policy_why [name=value ...]\n");
                return 2;
            }
            v[k] = atoi(eq + 1);
        }
        Row r;
        make(v, r);
        const urf_policy::reasons y = why_of(r);
        printf("%d %u %u\n", front_of(r) ? 1 : 0, y.why, y.advice);
        return 0;
    }
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
        all.rows += sums[t].rows, all.fronts += sums[t].fronts, all.nevers += sums[t].nevers, all.failures += sums[t].failures;
    }
    printf("rows %llu front %llu never %llu failures %llu\n", all.rows, all.fronts, all.nevers, all.failures);
    return all.failures ? 1 : 0;
}
