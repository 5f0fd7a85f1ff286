/*
 * urf_api.hip -- host side of the C ABI (include/urf.h): context, scratch
 * memory, kernel sequencing.  No CPU fallback: every entry point that
 * classifies fails with URF_ERR_NO_DEVICE / URF_ERR_HIP when there is no GPU.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <string>
#include <vector>
#if defined(__SSE2__)
#include <emmintrin.h>
#include <xmmintrin.h>
#endif

#include "urf.h"
#ifdef URF_ENABLE_TEST_HOOKS
#include "urf_test_hooks.h"
#endif
#include "urf_internal.hpp"
#include "urf_policy.hpp"
#include "urf_kernels.hpp"
#include "urf_front.hpp"
#include "urf_k_front_sectors.hpp"
#include "urf_k_front_outputs.hpp"
#include "urf_k_front_explain.hpp"
#include "urf_k_front_digest.hpp"

#include "urf_ctx.hpp"

/* The kernels of a call's fused family (urf_policy.hpp: urf_front_family), in one table.  An instance of the march and of the finish kernel
 * exists per curbPoints (the march twice: plain, and as the march of urf_set_front_multi_sector): the march per laser count -- 16, 32, 64, 128: the family's
 * `lasers` --, the finish kernel per width, because 64, 32 and 16 lasers share one that reads the count at run time (front_lsh).  The probe,
 * the transpose and the label kernel exist per width only. */
struct front_kernels {
    void (*probe)(urf_kargs, urf_dev_params);
    void (*transpose)(urf_kargs);
    void (*march)(urf_kargs, urf_dev_params);
    void (*finish)(urf_kargs, urf_dev_params, unsigned);
    void (*label)(urf_kargs, urf_dev_params);
};
static const struct {
    int cp;
    bool ms;
    decltype(front_kernels::march) march[4];
    decltype(front_kernels::finish) finish[2];
} FRONT_INSTANCES[] = {
    { 5, false, { k_front16, k_front32, k_front, k_front128 }, { k_front_finish, k_front_finish128 } },   /* the symbols of every front mode */
    { 5, true, { k_front16_ms, k_front32_ms, k_front_ms, k_front128_ms }, { k_front_finish, k_front_finish128 } },
#define URF_FRONT_CP_X(n) \
    { n, false, { k_front16_cp##n, k_front32_cp##n, k_front_cp##n, k_front128_cp##n }, { k_front_finish_cp##n, k_front_finish128_cp##n } },
    URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X
#define URF_FRONT_CP_X(n) \
    { n, true, { k_front16_ms_cp##n, k_front32_ms_cp##n, k_front_ms_cp##n, k_front128_ms_cp##n }, { k_front_finish_cp##n, k_front_finish128_cp##n } },
    URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)   /* (urf_set_front_multi_sector_curb_points) */
#undef URF_FRONT_CP_X
};
static front_kernels front_kernels_of(const urf_front_family& f)
{
    const auto* in = &FRONT_INSTANCES[0];   /* (a call without the fused kernels launches none of them) */
    for (const auto& i : FRONT_INSTANCES)
        if (i.cp == f.cp && i.ms == (f.ms != 0))
            in = &i;
    return { f.wide ? k_rows_probe128 : k_rows_probe, f.wide ? k_transpose128 : k_transpose, in->march[f.lasers], in->finish[f.wide],
             f.wide ? k_label_front128 : k_label_front };
}
/* ... and the one place where the 128-laser family's candidate lists (URF_FRONT128_CAND_CAP) take the place of the others' */
static void front_family_args(const urf_front_family& f, uint32_t max_points, urf_kargs& a)
{
    if (f.wide) {
        a.front_cand = a.front_cand128;
        a.front_all = a.front_all128;
        a.front_cand_cap = URF_FRONT128_CAND_CAP(max_points);
    }
}

/* the finish kernels' dynamic LDS for `tiles` tiles (above URF_FRONT_MAX_TILES: urf_set_front_long_sweeps has asked the device) */
static constexpr size_t urf_finish_lds_bytes(unsigned tiles)
{
    return (size_t)tiles * 384 + 2 * URF_FINISH_CHUNK * sizeof(urf_u2);
}
static_assert(urf_finish_lds_bytes(URF_FRONT_LONG_MAX_TILES) + sizeof(urf_finish_shared_t<URF_FRONT128_L>) <= 160u * 1024u, "a CU's LDS");
static_assert(URF_FRONT128_TILES2(URF_FRONT_LONG_MAX_TILES) == URF_FRONT_LONG_MAX_TILES, "an even number: k_front_finish128's layout is as large");

/* the call's part of the per-scan rule (urf_front_scan_rule): `rows`, the layout the records are counted in; sweep_n, a sweep's own length */
static urf_fx_call fx_call_of(const urf_run& r, bool rows, uint32_t sweep_n)
{
    const uint32_t L = (uint32_t)r.dp.p.channels;
    return urf_fx_call{ r.a.front, r.a.front_rows, r.a.front_cand_cap, rows ? 1u : 0u, (L == 16u || L == 32u || L == 64u || L == 128u) ? L : 0u,
                        r.planned.ms ? 1u : 0u, r.dp.p.curbPoints != 5 ? 1u : 0u, r.planned.call.why, sweep_n };
}
static void seq_drop(urf_ctx::slot_t& sl, unsigned i)
{
    urf_ctx::slot_t::seq_t& q = sl.seqs[i];
    if (q.exec)
        (void)hipGraphExecDestroy(q.exec);
    if (q.graph)
        (void)hipGraphDestroy(q.graph);
    q.exec = nullptr;
    q.graph = nullptr;
    sl.cache.drop(i);   /* (never while the slot's sweep is in flight) */
}

/* What the kernels of earlier calls reported, taken into the policy before a call's launches (never inside a stream capture: the first
 * row-major sighting lets the calls in flight on `st`, the stream the call launches on, finish -- what they handed back, possibly all
 * of their sweeps, says nothing about the calls to come -- and allocates the firing-order copies before the call takes its arguments). */
static void auto_apply(urf_ctx* c, uint32_t bits);   /* (urf_set_front_auto: the setters' bodies, below) */

int urf_policy::fold(urf_ctx* c, hipStream_t st)   /* (hipStream_t: ihipStream_t*) */
{
    if (front_mode != 0 && !front_rows && !rows_oom && flags[URF_FLAG_ROWS_SIGHTED]) {
        URF_HIP(c, hipStreamSynchronize(st));
        if (scratch_alloc(c, URF_SCR_ROW_MAJOR) == URF_OK) {
            set(front_rows, true);
            rows_probation = 16;
            forget_front();
            auto_start();   /* (what a pass counted in firing order says nothing about these sweeps) */
        } else {
            set(rows_oom, true);   /* (such sweeps keep to the general kernels) */
            c->last_error.clear();
        }
    }
    if (front_rows && flags[URF_FLAG_ROWS_TAKEN])
        set(rows_used, true);
    if (flags[URF_FLAG_LOOKAHEAD_FAILED])
        set(speculate, false);
    if (flags[URF_FLAG_HINT_FAILED])
        set(use_hint, false);
    if (flags[URF_FLAG_FRONT_HANDED_BACK])
        set(front_direct, true);
    if (flags[URF_FLAG_FRONT_ALL_HANDED_BACK] && !every_batch())
        set(front_off, true);
    /* urf_set_front_auto: the digest of the pass in flight, once its sequence word is the one the host handed to the pass (k_front_digest
     * stores it last, behind a system-scope fence) -- never by waiting: a digest that has not arrived is looked for at the next call */
    if (auto_on && auto_wait && auto_phase == URF_AUTO_LEARNING) {
        const uint32_t which = auto_wait - 1u;
        const volatile uint32_t* d = c->au.dig.p + (size_t)which * URF_DG_WORDS;
        if (d[URF_DG_SEQ] == auto_seq) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            uint32_t w[URF_DG_WORDS];
            for (unsigned k = 0; k < URF_DG_WORDS; k++)
                w[k] = d[k];
            auto_wait = 0;
            if (which == 0u || w[URF_DG_SCANS] != 0u) {   /* (a sweep without a result -- voided and run again --: discarded) */
                std::memcpy(auto_digest_words, w, sizeof w);
                const auto_step step = auto_digest(w, c->dp);
                auto_left_digest = auto_digest_left(w);
                auto_phase = step.phase;
                if (step.again)
                    auto_again++;
                if (step.apply)
                    auto_apply(c, step.apply);   /* (may allocate: before the call takes its arguments, outside any capture) */
            } else if (auto_explained) {
                auto_explained--;   /* (a pass that taught nothing does not count: at most five per new start that do) */
            }
        }
    }
    return URF_OK;
}

/* star_shaped_search.cpp:32-66 beam_init: per-sector constants of the
 * rectangular beam; `fi` is a float, so tan/sin/cos(fi) are the float
 * overloads and tan(0.5*M_PI - fi) is the double one. */
static void beam_init(std::vector<urf_beam>& beams, int rep, float width)
{
    beams.resize((size_t)rep);
    const float off = (float)(0.5 * (double)width);
    for (int i = 0; i < rep; i++) {
        const float fi = (float)((double)(i * 2) * M_PI / (double)rep);
        if (std::fabs(std::tan(fi)) > 1) {
            beams[i].yx = 1;
            beams[i].d = (float)std::tan(0.5 * M_PI - (double)fi);
            beams[i].o = std::fabs(off / std::sin(fi));
        } else {
            beams[i].yx = 0;
            beams[i].d = std::tan(fi);
            beams[i].o = std::fabs(off / std::cos(fi));
        }
    }
}

/* x_zero_method.cpp:58-61 / z_zero_method.cpp:63-66 test "alpha <= angleFilter" with alpha = (float)((double)(acosf(b) * 180.0f) /
 * M_PI), b the clamped cosine.  alpha falls (weakly) as b grows -- checked for EVERY float of [-1, 1] against include/urf_libm.h's
 * acosf by tools/check_acos_threshold.c, together with the bisection below for fourteen filter angles -- so the test is "b >= T" with
 * T = the smallest float of [-1, 1] whose alpha passes: no arc cosine on the device (a fifth of the candidate chain of k_ring).  A NaN
 * cosine fails either form.  Returns 2 when no b passes. */
static float urf_angle_threshold(float angle_filter)
{
    auto alpha_of = [](float b) { return (float)((double)(urf_acosf(b) * 180.0f) / M_PI); };   /* (IEEE division: what urf_div_pi equals) */
    auto from_key = [](uint32_t k) {   /* the floats of [-1, 1] in ascending order */
        const uint32_t one = 0x3f800000u;
        const uint32_t u = k <= one ? 0x80000000u | (one - k) : k - one - 1u;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    if (!(alpha_of(1.0f) <= angle_filter))
        return 2.0f;
    uint32_t lo = 0, hi = 2u * 0x3f800000u + 1u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (alpha_of(from_key(mid)) <= angle_filter)
            hi = mid;
        else
            lo = mid + 1;
    }
    return from_key(lo);
}

static int upload_params(urf_ctx* c)
{
    const urf_params& p = c->params;
    urf_dev_params& dp = c->dp;
    dp.p = p;
    dp.slope_param = (float)((double)p.angleFilter3 * (M_PI / 180));   /* star_shaped_search.cpp:160 */
    dp.Kfi = (float)((double)p.sectors / (2 * M_PI));                  /* star_shaped_search.cpp:65 */
    dp.fwd_limit = 360.0f - p.beamZone;                                /* blind_spots.cpp:68 */
    dp.bwd_limit = 0.0f + p.beamZone;                                  /* blind_spots.cpp:177 */
    dp.inv_cp = 1.0f / (float)p.curbPoints;                            /* z_zero_method.cpp:52 */
    dp.x_angle_thr = urf_angle_threshold(p.angleFilter1);
    dp.z_angle_thr = urf_angle_threshold(p.angleFilter2);
    /* keys 0..K-1 plus "none" (mapped to K) must be distinguishable */
    dp.sec_keybits = 1;
    while ((1u << dp.sec_keybits) <= (unsigned)p.sectors)
        dp.sec_keybits++;
    dp.ring_keybits = 1;
    while ((1u << dp.ring_keybits) <= (unsigned)p.channels)
        dp.ring_keybits++;
    dp.exp_flags = c->debug_flags;
    dp.sector_margin = URF_FAST_SECTOR_ERR * (p.sectors > 360 ? (float)p.sectors / 360.0f : 1.0f);
    std::vector<urf_beam> beams;
    beam_init(beams, p.sectors, p.beam_width);
    URF_HIP(c, hipMemcpyAsync(c->d_beams, beams.data(), beams.size() * sizeof(urf_beam), hipMemcpyHostToDevice, c->stream));
    URF_HIP(c, hipStreamSynchronize(c->stream));   /* `beams` is a stack object */
    return URF_OK;
}

extern "C" int urf_create(urf_ctx** out, int device_id, uint32_t max_points, uint32_t max_batch)
{
    if (!out || max_points == 0 || max_batch == 0)
        return URF_ERR_INVALID_ARG;
    *out = nullptr;
    const unsigned long long max_tiles = ((unsigned long long)max_points + URF_TILE - 1) / URF_TILE;
    const unsigned long long sstride = max_tiles * URF_TILE + URF_SCAN_PAD;
    if (max_tiles > URF_MAX_TILES || sstride * max_batch >= (1ull << 32))
        return URF_ERR_CAPACITY;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev)
        return URF_ERR_NO_DEVICE;
    urf_ctx* c = new urf_ctx();
    c->device = device_id;
    c->max_points = max_points;
    c->max_batch = max_batch;
    c->max_tiles = (uint32_t)max_tiles;
    c->sstride = (uint32_t)sstride;
    for (unsigned i = 0; i < 256; i++)
        c->dense_map[i] = c->dense_elev.identity[i] = (uint8_t)i;
    (void)urf_set_dense_elevations(c, nullptr, 0);   /* (no table: the rest of dense_elev) */
    int rc = URF_OK;
    auto fail = [&](int code) {
        urf_destroy(c);
        return code;
    };
    if (hipSetDevice(device_id) != hipSuccess)
        return fail(URF_ERR_NO_DEVICE);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
        return fail(URF_ERR_HIP);
    c->stream = c->own_stream;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_cus = (unsigned)prop.multiProcessorCount;
    }
    urf_default_params(&c->params);
    std::memset(&c->k, 0, sizeof(c->k));
    std::memset(&c->last.run.a, 0, sizeof(c->last.run.a));
    urf_kargs& k = c->k;
    k.front_cand_cap = max_points / 8 > 4096 ? max_points / 8 : 4096;
    if ((rc = scratch_alloc(c, URF_SCR_ALWAYS)) != URF_OK || (rc = dev_alloc(c, &c->offsets_copy, (size_t)max_batch + 1)) != URF_OK ||
        (rc = dev_alloc(c, &c->compact_cnt, (size_t)max_batch * c->max_tiles * 4)) != URF_OK ||
        (rc = dev_alloc(c, &c->d_newY, (size_t)max_points)) != URF_OK || (rc = dev_alloc(c, &c->d_beams, (size_t)URF_MAX_SECTORS)) != URF_OK)
        return fail(rc);
    {
        urf_wu* tab = nullptr;
        const size_t nt = (size_t)max_points + 32;
        if ((rc = dev_alloc(c, &tab, nt)) != URF_OK)
            return fail(rc);
        hipLaunchKernelGGL(k_walk_table, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, tab, (unsigned)nt);
        k.walk_tab = tab;
    }
    k.sstride = c->sstride;
    if (const char* e = std::getenv("URF_FRONT_TPB"))   /* tuning experiments: tiles per block of k_front */
        c->pol.front_tpb = (uint32_t)std::atoi(e) > 0 ? (uint32_t)std::atoi(e) : c->pol.front_tpb;
    {
        void* hp = nullptr;
        if (hipHostMalloc(&hp, URF_FLAG_WORDS * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess)
            return fail(URF_ERR_HIP);
        c->pol.flags = (uint32_t*)hp;
        std::memset(hp, 0, URF_FLAG_WORDS * sizeof(uint32_t));
        if (hipMemset(k.ring_hint, 0, URF_ASYNC_SLOTS * sizeof(uint32_t)) != hipSuccess)
            return fail(URF_ERR_HIP);
        void* dp_ = nullptr;
        if (hipHostGetDevicePointer(&dp_, hp, 0) != hipSuccess)
            return fail(URF_ERR_HIP);
        k.flags = (uint32_t*)dp_;
    }
    /* x_zero_method.cpp:24-27: newY[j] = newY[j-1] + 0.0100 (float += double), a
     * data-independent table shared by all rings */
    {
        std::vector<float> newY(max_points);
        newY[0] = 0.0f;
        for (uint32_t j = 1; j < max_points; j++)
            newY[j] = (float)((double)newY[j - 1] + 0.0100);
        if (hipMemcpy(c->d_newY, newY.data(), newY.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return fail(URF_ERR_HIP);
    }
    k.newY = c->d_newY;
    k.beams = c->d_beams;
    if ((rc = upload_params(c)) != URF_OK)
        return fail(rc);
    *out = c;
    return URF_OK;
}

extern "C" int urf_destroy(urf_ctx* c)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->own_stream)
        (void)hipStreamSynchronize(c->own_stream);
    if (c->side_stream) {
        (void)hipStreamSynchronize(c->side_stream);
        (void)hipStreamDestroy(c->side_stream);
        (void)hipEventDestroy(c->ev_fork);
        (void)hipEventDestroy(c->ev_join);
    }
    for (hipStream_t st : c->row_stream)
        if (st)
            (void)hipStreamSynchronize(st);
    for (auto& set : c->timing_events)
        for (hipEvent_t e : set)
            (void)hipEventDestroy(e);
    for (void* p : c->allocs)
        (void)hipFree(p);
    if (c->pol.flags)
        (void)hipHostFree(c->pol.flags);
    for (auto& sl : c->slots) {
        for (unsigned i = 0; i < URF_SWEEP_SEQS; i++)
            seq_drop(sl, i);
        if (sl.ev_done)
            (void)hipEventDestroy(sl.ev_done);
    }
    for (hipStream_t st : c->row_stream)
        if (st)
            (void)hipStreamDestroy(st);
    if (c->ev_main)
        (void)hipEventDestroy(c->ev_main);
    if (c->own_stream)
        (void)hipStreamDestroy(c->own_stream);
    delete c;   /* (the lazily sized buffers go with it: lazy_buf) */
    return URF_OK;
}

extern "C" int urf_set_params(urf_ctx* c, const urf_params* p)
{
    if (!c || !p)
        return URF_ERR_INVALID_ARG;
    const int rc = urf_validate_params(p);
    if (rc != URF_OK)
        return rc;
    URF_HIP(c, hipSetDevice(c->device));
    for (hipStream_t st : c->row_stream)
        if (st)
            URF_HIP(c, hipStreamSynchronize(st));   /* a sweep in flight on another row keeps its parameters */
    /* the ring counts of earlier calls say nothing about sweeps classified with OTHER parameters (region of interest, interval) */
    if (std::memcmp(&c->params, p, sizeof(*p)) != 0) {
        URF_HIP(c, hipMemsetAsync(c->k.ring_hint, 0, URF_ASYNC_SLOTS * sizeof(uint32_t), c->stream));
        c->pol.forget_front();   /* ... nor does what the fused front end made of them */
        c->pol.auto_start();     /* ... nor what urf_set_front_auto learned from them */
    }
    c->params = *p;
    c->pol.epoch++;
    return upload_params(c);
}

extern "C" int urf_get_params(const urf_ctx* c, urf_params* p)
{
    if (!c || !p)
        return URF_ERR_INVALID_ARG;
    *p = c->params;
    return URF_OK;
}

extern "C" int urf_set_stream(urf_ctx* c, void* hip_stream)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    c->pol.epoch++;
    c->fo_prep.seq = 0;   /* (what k_front_out_prep wrote on the stream before is not ordered in front of this one) */
    c->dn_inv_of = 0;     /* (nor what k_dense_inverse wrote) */
    return URF_OK;
}

extern "C" int urf_synchronize(urf_ctx* c)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));
    for (hipStream_t st : c->row_stream)   /* sweeps of the callback path in flight on other scratch rows */
        if (st)
            URF_HIP(c, hipStreamSynchronize(st));
    return URF_OK;
}

extern "C" int urf_enable_stage_capture(urf_ctx* c, int mode)
{
    if (!c || mode < 0 || mode > 2)
        return URF_ERR_INVALID_ARG;
    if (mode) {
        URF_HIP(c, hipSetDevice(c->device));
        const int rc = scratch_alloc(c, URF_SCR_CAPTURE);
        if (rc != URF_OK)
            return rc;
    }
    c->capture = mode;
    c->pol.epoch++;
    return URF_OK;
}

extern "C" int urf_callback_path_state(const urf_ctx* c, uint32_t* n_rerun, uint32_t* sequence)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    if (n_rerun)
        *n_rerun = c->n_rerun;
    const urf_policy& p = c->pol;
    if (sequence)
        *sequence = (p.speculate ? 1u : 0u) | (p.slot_lists ? 2u : 0u) | (p.slot_nan ? 4u : 0u) | (p.speculate && p.use_hint ? 8u : 0u) | (p.slot_ties ? 16u : 0u);
    return URF_OK;
}

extern "C" int urf_callback_path_preset(urf_ctx* c, uint32_t sequence_bits)
{
    if (!c || (sequence_bits & ~(2u | 4u | 16u)))
        return URF_ERR_INVALID_ARG;
    urf_policy& p = c->pol;   /* (a change rebuilds the captured sequences) */
    p.set(p.slot_lists, p.slot_lists || (sequence_bits & 2u) != 0);
    p.set(p.slot_nan, p.slot_nan || (sequence_bits & 4u) != 0);
    p.set(p.slot_ties, p.slot_ties || (sequence_bits & 16u) != 0);
    return URF_OK;
}

extern "C" double urf_ring_threshold_cot(double angle_deg)
{
    return urf_cot_deg(angle_deg);
}

/* by_auto: urf_set_front_auto's own application (auto_apply) -- everything the caller's setter does but the new start of the learning */
static int set_front_mode(urf_ctx* c, int mode, bool by_auto)
{
    if (!c || mode < 0 || mode > 3)
        return URF_ERR_INVALID_ARG;
    const bool fresh = mode != c->pol.front_mode || (mode != 0 && c->pol.want_ring_sorted);
    if (mode != c->pol.front_mode && mode != 0)   /* (a new start) */
        c->pol.forget_front();
    c->pol.set(c->pol.front_mode, mode);
    if (mode != 0)
        c->pol.set(c->pol.want_ring_sorted, false);   /* (a caller that asks for ring-sorted results again pays for them again) */
    if (fresh && !by_auto)
        c->pol.auto_start();
    return URF_OK;
}
extern "C" int urf_set_front_mode(urf_ctx* c, int mode)
{
    return set_front_mode(c, mode, false);
}

/* The on / off switches of the fused front end that plan() reads: `prepare` (may be null) runs when the switch is turned on, before anything
 * changes, and may refuse; a change is a new start (forget_front); turning a switch on, like urf_set_front_mode, ends want_ring_sorted. */
static int set_front_switch(urf_ctx* c, int on, bool urf_policy::*field, int (*prepare)(urf_ctx*), bool by_auto = false)
{
    if (!c || (on != 0 && on != 1))
        return URF_ERR_INVALID_ARG;
    if (on && prepare) {
        URF_HIP(c, hipSetDevice(c->device));
        const int rc = prepare(c);
        if (rc != URF_OK)
            return rc;
    }
    if ((on != 0) != c->pol.*field) {   /* (a new start) */
        c->pol.forget_front();
        if (!by_auto)
            c->pol.auto_start();
    }
    c->pol.set(c->pol.*field, on != 0);
    if (on)
        c->pol.set(c->pol.want_ring_sorted, false);
    return URF_OK;
}

/* the five switches, each with the URF_ADVICE_* bit that names it: the entry points below and auto_apply run the same row */
static int long_sweeps_lds(urf_ctx* c);
static int front_switch(urf_ctx* c, uint32_t advice_bit, int on, bool by_auto = false)
{
    switch (advice_bit) {
    case URF_ADVICE_LASERS128:   /* what the fused kernels size for 64 lanes, sized for 128: allocated once, with the first call that turns the switch on */
        return set_front_switch(c, on, &urf_policy::lasers128, [](urf_ctx* x) { return scratch_alloc(x, URF_SCR_LASERS128); }, by_auto);
    case URF_ADVICE_LONG_SWEEPS:
        return set_front_switch(c, on, &urf_policy::long_sweeps, long_sweeps_lds, by_auto);
    case URF_ADVICE_CURB_POINTS:
        return set_front_switch(c, on, &urf_policy::curb_points, nullptr, by_auto);
    case URF_ADVICE_MULTI_SECTOR:   /* the star records' sectors, one per scratch element: allocated once, with the first call that turns the switch on */
        return set_front_switch(c, on, &urf_policy::multi_sector, [](urf_ctx* x) { return scratch_alloc(x, URF_SCR_MULTI_SECTOR); }, by_auto);
    case URF_ADVICE_MULTI_SECTOR_CP:   /* (allocates nothing: front_skey comes with urf_set_front_multi_sector, without which this switch decides nothing) */
        return set_front_switch(c, on, &urf_policy::multi_sector_cp, nullptr, by_auto);
    }
    return URF_ERR_INVALID_ARG;
}

/* urf_set_front_auto applies advice: each bit through the code its setter runs, allocation included.  A bit that answers URF_ERR_OOM goes
 * to auto_refused, the error text is cleared and the caller goes on without it; bits are only ever turned on. */
static void auto_apply(urf_ctx* c, uint32_t bits)
{
    urf_policy& p = c->pol;
    for (const uint32_t bit : { URF_ADVICE_LASERS128, URF_ADVICE_LONG_SWEEPS, URF_ADVICE_CURB_POINTS, URF_ADVICE_MULTI_SECTOR, URF_ADVICE_MULTI_SECTOR_CP })
        if (bits & bit) {
            if (front_switch(c, bit, 1, true) == URF_OK) {
                p.auto_applied |= bit;
            } else {
                p.auto_refused |= bit;
                c->last_error.clear();
            }
        }
    if ((bits & URF_ADVICE_MODE_3) && set_front_mode(c, 3, true) == URF_OK)
        p.auto_applied |= URF_ADVICE_MODE_3;
}

/* Call-level advice, at the call itself: behind fold(), in front of plan() and of the call's arguments (a switch may allocate a scratch
 * group), outside any stream capture.  tiles, n_scans, capture: what plan() will read of the call. */
static void auto_at_call(urf_ctx* c, uint32_t tiles, uint32_t n_scans, uint32_t capture, bool slot)
{
    urf_policy& p = c->pol;
    if (!p.auto_on)
        return;
    urf_kargs a = c->k;
    a.tiles = tiles;
    a.n_scans = n_scans;
    a.capture = capture;
    urf_policy::reasons r = p.why(a, c->dp, slot, false);
    if (const uint32_t bits = p.auto_call(r.why, r.advice)) {
        auto_apply(c, bits);
        r = p.why(a, c->dp, slot, false);
    }
    p.auto_left = r.advice & URF_ADVICE_LEFT_MASK;
}

extern "C" int urf_set_front_lasers128(urf_ctx* c, int on)
{
    return front_switch(c, URF_ADVICE_LASERS128, on);
}

/* The finish kernels' dynamic LDS at URF_FRONT_LONG_MAX_TILES tiles: a device that does not grant a workgroup that much keeps the switch
 * off.  Measured on the MI355X: the HIP runtime grants a workgroup the whole 160 KiB without being asked -- a launch
 * with 110 592 B succeeds without hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize), and the call changes neither that nor
 * the occupancy below 129 tiles -- so the attribute is not set: this limit is the only condition. */
static int long_sweeps_lds(urf_ctx* c)
{
    int lds_max = 0;
    URF_HIP(c, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if ((size_t)lds_max < urf_finish_lds_bytes(URF_FRONT_LONG_MAX_TILES) + sizeof(urf_finish_shared_t<URF_FRONT128_L>)) {
        c->last_error = "urf_set_front_long_sweeps: the device grants a workgroup " + std::to_string(lds_max) + " bytes of LDS";
        return URF_ERR_OOM;
    }
    return URF_OK;
}
extern "C" int urf_set_front_long_sweeps(urf_ctx* c, int on)
{
    return front_switch(c, URF_ADVICE_LONG_SWEEPS, on);
}

extern "C" int urf_set_front_curb_points(urf_ctx* c, int on)
{
    return front_switch(c, URF_ADVICE_CURB_POINTS, on);
}

extern "C" int urf_set_front_multi_sector(urf_ctx* c, int on)
{
    return front_switch(c, URF_ADVICE_MULTI_SECTOR, on);
}

extern "C" int urf_set_front_multi_sector_curb_points(urf_ctx* c, int on)
{
    return front_switch(c, URF_ADVICE_MULTI_SECTOR_CP, on);
}

/* ---- urf_set_front_auto (include/urf.h) ------------------------------------------------------- */
static_assert(sizeof(urf_front_auto_info) == 64 && offsetof(urf_front_auto_info, digest_seq) == 24, "include/urf.h: the digest's eight words in k_front_digest's order");
/* Everything the learning pass will need, before any call launches it: nothing is allocated behind a call or inside a stream capture. */
static int auto_alloc(urf_ctx* c)
{
    const size_t passes = 1 + URF_ASYNC_SLOTS;
    int rc;
    if ((rc = grow(c, c->au.rec, ((size_t)c->max_batch + URF_ASYNC_SLOTS) * URF_FX_WORDS)) != URF_OK || (rc = grow(c, c->au.acc, passes * URF_DG_WORDS)) != URF_OK)
        return rc;
    mapped_buf& m = c->au.dig;
    if (!m.p) {
        void *hp = nullptr, *dp_ = nullptr;
        URF_HIP(c, hipHostMalloc(&hp, passes * URF_DG_WORDS * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
        m.p = (uint32_t*)hp;
        m.cap = passes * URF_DG_WORDS;
        std::memset(m.p, 0, m.cap * sizeof(uint32_t));
        URF_HIP(c, hipHostGetDevicePointer(&dp_, hp, 0));
        m.dev = (uint32_t*)dp_;
    }
    return URF_OK;
}

extern "C" int urf_set_front_auto(urf_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1))
        return URF_ERR_INVALID_ARG;
    urf_policy& p = c->pol;
    if (on) {
        URF_HIP(c, hipSetDevice(c->device));
        const int rc = auto_alloc(c);
        if (rc != URF_OK) {
            c->au.dig.release();   /* (all of it or none: a later call tries again) */
            c->au.rec.release();
            c->au.acc.release();
            return rc;
        }
        p.auto_on = true;
        p.auto_left = 0;
        p.auto_start();   /* (turning it on again is a new start; a pass still in flight finishes into buffers that stay) */
    } else {
        p.auto_on = false;
        p.auto_phase = URF_AUTO_IDLE;
        p.auto_wait = 0;
    }
    return URF_OK;
}

extern "C" int urf_front_auto_query(urf_ctx* c, urf_front_auto_info* out)
{
    if (!c || !out)
        return URF_ERR_INVALID_ARG;
    const int rc = urf_synchronize(c);
    if (rc != URF_OK)
        return rc;
    const urf_policy& p = c->pol;
    std::memset(out, 0, sizeof *out);
    out->applied = p.auto_applied;
    if (!p.auto_on)
        return URF_OK;
    out->on = 1u;
    out->phase = p.auto_phase;
    out->refused = p.auto_refused;
    out->left = p.auto_left | p.auto_left_digest;
    out->explained_calls = p.auto_explained;
    /* the pass in flight has completed with the stream: its digest as it stands, else the one fold() took last */
    const uint32_t* d = p.auto_digest_words;
    if (p.auto_wait && c->au.dig.p[(size_t)(p.auto_wait - 1u) * URF_DG_WORDS + URF_DG_SEQ] == p.auto_seq)
        d = c->au.dig.p + (size_t)(p.auto_wait - 1u) * URF_DG_WORDS;
    std::memcpy(&out->digest_seq, d, URF_DG_WORDS * sizeof(uint32_t));
    return URF_OK;
}

extern "C" int urf_set_front_outputs(urf_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1))
        return URF_ERR_INVALID_ARG;
    c->pol.front_outputs = on != 0;   /* (the read-outs' scratch grows with their first use: readouts_of_last) */
    return URF_OK;
}

extern "C" int urf_front_scans(urf_ctx* c, uint32_t* n_fused)
{
    if (!c || !n_fused)
        return URF_ERR_INVALID_ARG;
    *n_fused = 0;
    if (!c->last.run.a.front)   /* (or no call yet) */
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));   /* (a sweep of the callback path has been waited for: its row is at rest) */
    std::vector<uint32_t> ok(c->last.scans);
    URF_HIP(c, hipMemcpy(ok.data(), c->last.run.a.front_ok, ok.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t v : ok)
        *n_fused += v ? 1u : 0u;
    return URF_OK;
}

extern "C" int urf_enable_kernel_timing(urf_ctx* c, int on)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    c->timing = on != 0;
    c->pol.epoch++;
    return URF_OK;
}

extern "C" const char* urf_kernel_name(int i)
{
    static const char* names[URF_NUM_KERNELS] = { "k_ring_table", "k_split", "k_index", "k_star_sort",
                                                  "k_star_walk", "k_ring", "k_beams", "k_label" };
    return (i >= 0 && i < URF_NUM_KERNELS) ? names[i] : "";
}

extern "C" int urf_kernel_timing(urf_ctx* c, double* ms_sum, uint32_t* n_calls)
{
    if (!c || !ms_sum || !n_calls)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));
    for (hipStream_t st : c->row_stream)   /* (with timing on, a sweep of the callback path records its events on its row's stream) */
        if (st)
            URF_HIP(c, hipStreamSynchronize(st));
    for (size_t i = 0; i < c->timing_used; i++) {
        auto& set = c->timing_events[i];
        for (int k = 0; k < URF_NUM_KERNELS; k++) {
            float ms = 0.f;
            URF_HIP(c, hipEventElapsedTime(&ms, set[k], set[k + 1]));
            ms_sum[k] += (double)ms;
        }
        (*n_calls)++;
    }
    c->timing_used = 0;   /* the events stay allocated and are recorded again by the next calls */
    return URF_OK;
}

extern "C" const char* urf_last_error(const urf_ctx* c) { return c ? c->last_error.c_str() : ""; }

/* Work on the context's stream that reads or writes scratch (any row), the SoA staging or the results of
 * the last call must come after the sweeps of the callback path that are still in flight on OTHER
 * streams (a batch call overwrites their rows; urf_read_stage / urf_ordered_indices /
 * urf_marker_points read them) ... */
static int order_after_slots(urf_ctx* c)
{
    for (auto& sl : c->slots)
        if (sl.pending && sl.ev_done)
            URF_HIP(c, hipStreamWaitEvent(c->stream, sl.ev_done, 0));   /* (a no-op for a slot that ran on `stream` itself) */
    c->main_seq++;
    return URF_OK;
}
/* ... and a sweep launched on a row's own stream must come after whatever the context's stream still
 * has to do with that row or the staging arrays. */
static int order_row_after_main(urf_ctx* c, uint32_t row, hipStream_t st)
{
    if (st == c->stream || c->row_seen[row] == c->main_seq)
        return URF_OK;
    if (!c->ev_main)
        URF_HIP(c, hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    URF_HIP(c, hipEventRecord(c->ev_main, c->stream));
    URF_HIP(c, hipStreamWaitEvent(st, c->ev_main, 0));
    c->row_seen[row] = c->main_seq;
    return URF_OK;
}

/* urf_set_front_auto's learning pass behind a call that launched the fused kernels, on the call's stream: k_front_explain as
 * urf_front_explain launches it -- layout 1 exactly when the call's sequence held the rows' probe and transpose --, then k_front_digest
 * into digest `which` (0: a batch call's, 1 + i: slot i's).  rec_row: the first row of au.rec the call's records take; sweep_n: a sweep's
 * own length.  One pass is in flight at a time; while learning is over, or the call kept the general kernels: nothing. */
static int auto_pass(urf_ctx* c, const urf_run& r, hipStream_t st, uint32_t which, uint32_t rec_row, uint32_t sweep_n)
{
    urf_policy& p = c->pol;
    const urf_kargs& a = r.a;
    if (!p.auto_on || p.auto_phase != URF_AUTO_LEARNING || p.auto_wait || !a.front || !c->au.dig.p)
        return URF_OK;
    const uint32_t n = a.n_scans;
    uint32_t* const rec = c->au.rec.p + (size_t)rec_row * URF_FX_WORDS;
    uint32_t* const acc = c->au.acc.p + (size_t)which * URF_DG_WORDS;
    const bool rows = a.front_rows != 0u;
    URF_HIP(c, hipMemsetAsync(rec, 0, (size_t)n * URF_FX_WORDS * sizeof(uint32_t), st));
    URF_HIP(c, hipMemsetAsync(acc, 0, URF_DG_WORDS * sizeof(uint32_t), st));
    if (++p.auto_seq == 0u)
        p.auto_seq = 1u;   /* (0: what a fresh digest slot holds) */
    hipLaunchKernelGGL(k_front_explain, dim3(a.tiles, n), dim3(64), 0, st, a, r.dp, rows ? 1u : 0u, rec);
    hipLaunchKernelGGL(k_front_digest, dim3((n + 255u) / 256u), dim3(256), 0, st, a, fx_call_of(r, rows, sweep_n), rec, acc,
                       c->au.dig.dev + (size_t)which * URF_DG_WORDS, p.auto_seq);
    URF_HIP(c, hipGetLastError());
    p.auto_wait = which + 1u;
    p.auto_explained++;
    return URF_OK;
}

/* ---- the pipeline ---------------------------------------------------------- */
/* One call of the pipeline: a call of the public batch entry points (stream == nullptr: row 0 onwards, the context's stream), or one
 * sweep of the callback path on its row and stream.  Either caller publishes it as "the last call" (publish_last): a batch call at once,
 * a sweep when it is waited for. */
struct urf_call {
    const float *x, *y, *z;
    const uint32_t* offsets;        /* ragged: [n_scans + 1]; else nullptr */
    uint32_t n_per_scan, max_len, n_scans;
    uint8_t* labels;
    urf_scan_info* info;            /* the scans' summaries are copied there (may be nullptr) */
    uint32_t row = 0;
    hipStream_t stream = nullptr;
    /* the parameters and capture mode a voided sweep was SUBMITTED with (its rerun, urf_classify_pc2_wait); nullptr / -1: the context's */
    const urf_dev_params* dp = nullptr;
    int capture = -1;
    bool general_only = false;      /* no fused kernels (last_call) */
};

/* k_front_finish's first part runs on a stream of its own (run_pipeline).  Makes the stream and its two events once -- all three or none:
 * a later call tries again -- and lets the stream wait for `st`; false when it cannot. */
static bool side_fork(urf_ctx* c, hipStream_t st)
{
    if (!c->side_stream) {
        hipStream_t s = nullptr;
        hipEvent_t f = nullptr, j = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&f, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&j, hipEventDisableTiming) == hipSuccess) {
            c->side_stream = s;
            c->ev_fork = f;
            c->ev_join = j;
        } else {
            if (f)
                (void)hipEventDestroy(f);
            if (s)
                (void)hipStreamDestroy(s);
        }
    }
    return c->side_stream && hipEventRecord(c->ev_fork, st) == hipSuccess && hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) == hipSuccess;
}

/* The launch sequence of one call as the policy plans it; what it ran with -- arguments, parameters, the policy's words -- goes to `out`,
 * last of all and only for a call that succeeded and was not empty (call.dp may point into `out`, the call's values may come from out.a:
 * the two reruns) */
static int run_pipeline(urf_ctx* c, const urf_call& call, urf_run& out)
{
    if (!call.x || !call.y || !call.z || !call.labels)
        return URF_ERR_INVALID_ARG;
    const uint32_t n_scans = call.n_scans;
    if (n_scans == 0)
        return URF_OK;
    if (call.row + n_scans > c->max_batch || call.max_len > c->max_points)
        return URF_ERR_CAPACITY;
    URF_HIP(c, hipSetDevice(c->device));
    const bool slot = call.stream != nullptr;
    hipStream_t st = slot ? call.stream : c->stream;
    if (!slot) {   /* (a sweep of the callback path: urf_classify_pc2_async has done both, outside its stream capture) */
        int rc = order_after_slots(c);
        if (rc == URF_OK)
            rc = c->pol.fold(c, st);   /* (may allocate the row-major group: before the arguments are taken) */
        if (rc != URF_OK)
            return rc;
        if (c->pol.auto_on && !call.general_only)   /* urf_set_front_auto: the call's advice, applied before it is planned (may allocate a scratch group) */
            auto_at_call(c, std::max<uint32_t>((call.max_len + URF_TILE - 1) / URF_TILE, 1u), n_scans, (uint32_t)(call.capture >= 0 ? call.capture : c->capture), false);
    }
    urf_run run;
    urf_kargs& a = run.a;
    a = kargs_row(c, call.row);
    a.x = call.x;
    a.y = call.y;
    a.z = call.z;
    a.offsets = nullptr;
    if (call.offsets) {
        /* the context keeps its own copy: the entry points that look at this call's results later
         * (urf_read_stage, urf_ordered_indices, urf_marker_points) must not depend on the caller
         * keeping d_offsets alive.  Scratch memory is indexed by scan, never by these offsets. */
        if (call.offsets != c->offsets_copy)   /* (last_call runs the last call again with the copy itself) */
            URF_HIP(c, hipMemcpyAsync(c->offsets_copy, call.offsets, ((size_t)n_scans + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        a.offsets = c->offsets_copy;
    }
    a.n_per_scan = call.n_per_scan;
    a.n_scans = n_scans;
    a.max_len = call.max_len;
    a.tiles = (call.max_len + URF_TILE - 1) / URF_TILE;
    if (a.tiles == 0)
        a.tiles = 1;
    a.sstride = c->sstride;
    a.capture = (uint32_t)(call.capture >= 0 ? call.capture : c->capture);
    a.labels = call.labels;
    if (a.capture != 1) {
        a.rd2 = nullptr;
        a.caz = nullptr;
    }
    run.dp = call.dp ? *call.dp : c->dp;
    const urf_dev_params& dp = run.dp;
    const unsigned C = (unsigned)dp.p.channels, K = (unsigned)dp.p.sectors;
    const bool star = dp.p.star_shaped_method != 0;
    const dim3 g_tiles(a.tiles, n_scans), g_scan(n_scans);
    c->pol.plan(a, dp, slot, call.general_only);
    run.planned = urf_planned{ c->pol.why(a, dp, slot, call.general_only), c->pol.ms_ok(dp) };   /* (host words for urf_front_explain: decides nothing) */
    if (!slot)
        c->pol.probation_batch(a);

    std::vector<hipEvent_t>* ev = nullptr;
    if (c->timing) {
        if (c->timing_used == c->timing_events.size()) {
            c->timing_events.emplace_back(URF_NUM_KERNELS + 1);
            for (hipEvent_t& e : c->timing_events.back())
                URF_HIP(c, hipEventCreate(&e));
        }
        ev = &c->timing_events[c->timing_used++];
    }
    int stage = 0;
    auto mark = [&]() {
        if (ev)
            (void)hipEventRecord((*ev)[stage], st);
        stage++;
    };
    mark();
    const urf_front_family fam = urf_front_family_of(a.front, a.front_lsh, a.front_rows, a.front_ms, a.tiles, dp.p.curbPoints);
    const front_kernels fk = front_kernels_of(fam);
    front_family_args(fam, c->max_points, a);
    if (fam.rows)
        hipLaunchKernelGGL(fk.probe, g_scan, dim3(256), 0, st, a, dp);
    hipLaunchKernelGGL(k_ring_table, g_scan, dim3(URF_TABLE_THREADS), 0, st, a, dp);
    mark();
    if (fam.rows)
        hipLaunchKernelGGL(fk.transpose, g_tiles, dim3(256), 0, st, a);
    if (a.front) {   /* (a tile is URF_TILE points, whatever the laser count: URF_TILE / L firings) */
        const dim3 g_front((a.tiles + a.front_tpb - 1) / a.front_tpb, n_scans);
        hipLaunchKernelGGL(fk.march, g_front, dim3(64), 0, st, a, dp);
    }
    if (a.front_lists) {   /* what k_front handed back (normally nothing) */
        hipLaunchKernelGGL(k_table_repair, g_scan, dim3(URF_TABLE_THREADS), 0, st, a, dp, 1u);
        hipLaunchKernelGGL(k_split_list, dim3(c->n_cus * 2), dim3(URF_TILE_THREADS), urf_split_lds_bytes(C, K, star), st, a, dp);
    } else {
        hipLaunchKernelGGL(k_split, g_tiles, dim3(URF_TILE_THREADS), urf_split_lds_bytes(C, K, star), st, a, dp);
    }
    if ((a.table_lookahead || a.front_rows) && !(a.optimistic & URF_OPT_NO_REPAIR)) {   /* normally both find nothing to do */
        hipLaunchKernelGGL(k_table_repair, g_scan, dim3(URF_TABLE_THREADS), 0, st, a, dp, 0u);
        hipLaunchKernelGGL(k_split_repair, dim3(c->n_cus), dim3(URF_TILE_THREADS), urf_split_lds_bytes(C, K, star), st, a, dp);
    }
    /* the tiles of the scans k_front*_ms kept: their star records by sector, their tsoff rows (a scan that was handed back: k_split's) */
    if (a.front_ms)
        hipLaunchKernelGGL(k_front_sectors, g_tiles, dim3(URF_FSEC_THREADS), 0, st, a, dp);
    mark();
    /* k_front_finish's first part (positions, the detectors' candidates and their marks) depends on nothing behind k_front: it goes to a
     * stream of its own and runs NEXT TO k_index, the star-shaped search's sort and walk -- it waits for scattered loads (0.18 ms on its
     * own), they are bound by vector issue.  With the per-kernel event brackets on (urf_enable_kernel_timing) everything stays on one
     * stream, so that the brackets add up to the step. */
    bool side = false, part1 = false;
    const size_t finish_lds = urf_finish_lds_bytes(fam.finish_tiles);
    if (a.front && !ev && !slot && side_fork(c, st)) {
        hipLaunchKernelGGL(fk.finish, g_scan, dim3(URF_FINISH_THREADS), finish_lds, c->side_stream, a, dp, 1u);
        part1 = true;
        side = hipEventRecord(c->ev_join, c->side_stream) == hipSuccess;
        if (!side)   /* (cannot be joined by an event: wait for it here) */
            (void)hipStreamSynchronize(c->side_stream);
    }
    hipLaunchKernelGGL(k_index, g_scan, dim3(256), 0, st, a, dp);
    mark();
    /* k_star_ties: persistent one-wave workgroups (32 KB of LDS: four per CU) over a list that holds one sector in a hundred of
     * a sensor's sweep and nothing of a benchmark cloud */
    const unsigned tie_grid = K * n_scans < c->n_cus * 4u ? K * n_scans : c->n_cus * 4u;
    const unsigned tie_grid_small = K * n_scans < c->n_cus * 16u ? K * n_scans : c->n_cus * 16u;   /* (8 KB of LDS per wave) */
    if (star) {
        const dim3 g_sec(K, n_scans);
        hipLaunchKernelGGL(k_star_sort_small, g_sec, dim3(URF_STAR_THREADS), 0, st, a, dp);
        /* persistent workgroups over the (normally empty) work lists of oversized sectors */
        if (!(a.optimistic & URF_OPT_NO_LISTS)) {
            hipLaunchKernelGGL(k_star_sort_mid, dim3(c->n_cus * (URF_MID_WAVES * 256 / URF_STAR_MID_THREADS)), dim3(URF_STAR_MID_THREADS), 0, st,
                               a, dp);   /* as many workgroups as are resident */
            hipLaunchKernelGGL(k_star_sort_big, dim3(c->n_cus * 2), dim3(256), 0, st, a, dp);
            hipLaunchKernelGGL(k_star_sort_runs, dim3(c->n_cus * 20), dim3(URF_STAR_THREADS), 0, st, a, dp);   /* (five waves per SIMD) */
        }
        /* sectors whose sorted prefix holds equal planar ranges of different heights (URF_TIE_FLAG): the order libstdc++'s std::sort
         * leaves them in.  Benchmark clouds hold none (the kernel returns at once); a real sensor's sweep holds equal ranges in
         * every sector, but nearly all of them between twins (one height), which only the second pass below cares about. */
        if (!(a.optimistic & URF_OPT_NO_TIES)) {
            hipLaunchKernelGGL((k_star_ties<false, URF_TIE_SMALL>), dim3(tie_grid_small), dim3(64), 0, st, a, dp);
            hipLaunchKernelGGL((k_star_ties<false, URF_TIE_CAP>), dim3(tie_grid), dim3(64), 0, st, a, dp);
        }
    }
    mark();   /* "k_star_sort" = the three sort kernels (mid / big run over normally empty work lists) */
    if (star) {
        if (n_scans <= URF_WALK_FEW_SCANS)   /* an empty device: three waves per 64 sectors, one chunk apart */
            hipLaunchKernelGGL(k_star_walk_few, dim3((K + 63) / 64, n_scans), dim3(URF_WALK_FEW_THREADS), 0, st, a, dp);
        else
            hipLaunchKernelGGL(k_star_walk, dim3((K + 63) / 64, n_scans), dim3(64), 0, st, a, dp);
        /* second pass of k_star_ties: the sectors in which the walk stopped at a point with a twin behind it (URF_TIE_POST) */
        if (!(a.optimistic & URF_OPT_NO_TIES)) {
            hipLaunchKernelGGL((k_star_ties<true, URF_TIE_SMALL>), dim3(tie_grid_small), dim3(64), 0, st, a, dp);
            hipLaunchKernelGGL((k_star_ties<true, URF_TIE_CAP>), dim3(tie_grid), dim3(64), 0, st, a, dp);
        }
    }
    mark();
    const dim3 g_ring(C, n_scans);
    if (a.front_lists)
        hipLaunchKernelGGL(k_ring_list, dim3(c->n_cus * 8), dim3(URF_RING_THREADS), (2 * (size_t)a.tiles + 1) * sizeof(unsigned), st, a, dp);
    else if (dp.p.curbPoints == 5)   /* the reference's default: four points per thread, z only */
        hipLaunchKernelGGL(k_ring, g_ring, dim3(URF_RING_THREADS), (2 * (size_t)a.tiles + 1) * sizeof(unsigned), st, a, dp);
    else
        hipLaunchKernelGGL(k_ring_general, g_ring, dim3(URF_RING_THREADS), (2 * (size_t)a.tiles + 1) * sizeof(unsigned), st, a, dp);
    if (a.front) {
        if (side && hipStreamWaitEvent(st, c->ev_join, 0) != hipSuccess)
            (void)hipStreamSynchronize(c->side_stream);
        hipLaunchKernelGGL(fk.finish, g_scan, dim3(URF_FINISH_THREADS), finish_lds, st, a, dp, part1 ? 2u : 0u);   /* (2: the star-shaped hits, the hand-over to k_beams) */
    }
    /* the rings that hold a point with a NaN azimuth (k_split listed them: normally none, the kernel returns at once) */
    if (!(a.optimistic & URF_OPT_NO_NAN))
        hipLaunchKernelGGL(k_nan_rings, dim3(32), dim3(256), URF_NAN_LDS * sizeof(unsigned long long), st, a, dp);
    mark();
    hipLaunchKernelGGL(k_beams, g_scan, dim3(URF_BEAM_THREADS), (size_t)C * (24 * sizeof(unsigned) + URF_CURB_LIST * sizeof(float)), st, a, dp);
    mark();
    if (a.front_lists)
        hipLaunchKernelGGL(k_label_list, dim3(c->n_cus * 4), dim3(URF_LABEL_TILE_THREADS), 0, st, a, dp);
    else
        hipLaunchKernelGGL(k_label, g_tiles, dim3(URF_LABEL_TILE_THREADS), 0, st, a, dp);
    if (a.front)
        hipLaunchKernelGGL(fk.label, g_tiles, dim3(URF_LABEL_TILE_THREADS), 0, st, a, dp);
    mark();
    URF_HIP(c, hipGetLastError());
    if (call.info)
        URF_HIP(c, hipMemcpyAsync(call.info, a.info, (size_t)n_scans * sizeof(urf_scan_info), hipMemcpyDeviceToDevice, st));
    if (!slot && !call.general_only) {   /* (a sweep of the callback path: urf_classify_pc2_async, behind its sequence) */
        const int rc = auto_pass(c, run, st, 0u, call.row, 0u);
        if (rc != URF_OK)
            return rc;
    }
    out = run;
    return URF_OK;
}

static void publish_last(urf_ctx* c, int kind, uint32_t scans, const urf_run& run, uint32_t row = 0, uint64_t gen = 0)
{
    c->last = urf_last_call{ kind, scans, run, row, gen };
    c->last_seq++;
}

/* a call of the public batch entry points: published after a successful call that was not empty (an empty one leaves the last call as it was) */
static int classify_batch(urf_ctx* c, int kind, const urf_call& call)
{
    urf_run run;
    const int rc = run_pipeline(c, call, run);
    if (rc == URF_OK && call.n_scans)
        publish_last(c, kind, call.n_scans, run);
    return rc;
}

extern "C" int urf_classify_batch_soa(urf_ctx* c, const float* d_x, const float* d_y, const float* d_z,
                                      uint32_t n_per_scan, uint32_t n_scans, uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    return classify_batch(c, URF_LAST_SOA, urf_call{ d_x, d_y, d_z, nullptr, n_per_scan, n_per_scan, n_scans, d_labels, d_info });
}

extern "C" int urf_classify_batch_soa_ragged(urf_ctx* c, const float* d_x, const float* d_y, const float* d_z,
                                             const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                             uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c || !d_offsets)
        return URF_ERR_INVALID_ARG;
    return classify_batch(c, URF_LAST_SOA, urf_call{ d_x, d_y, d_z, d_offsets, 0, max_len, n_scans, d_labels, d_info });
}

static int ensure_soa_staging(urf_ctx* c)
{
    const size_t n = (size_t)c->max_points * c->max_batch;
    int rc;
    if ((rc = grow(c, c->sx, n)) != URF_OK || (rc = grow(c, c->sy, n)) != URF_OK)
        return rc;
    return grow(c, c->sz, n);
}

/* field offsets of a PointCloud2 record: every FLOAT32 field must lie inside the record
 * (evaluated in 64 bits: the offsets come from an untrusted wire message) */
static bool pc2_layout_ok(uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z)
{
    const uint64_t ps = point_step;
    return ps >= 4 && (uint64_t)off_x + 4 <= ps && (uint64_t)off_y + 4 <= ps && (uint64_t)off_z + 4 <= ps;
}

/* PointCloud2 batches: the records [0, n_total) unpacked into the SoA staging at their own indices, then the pipeline (ragged: with
 * the caller's offsets, which index records and staging alike) */
static int classify_batch_pc2(urf_ctx* c, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total, uint32_t n_per_scan,
                              uint32_t max_len, uint32_t n_scans, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                              uint8_t* d_labels, urf_scan_info* d_info)
{
    if (n_scans == 0)
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    int rc = ensure_soa_staging(c);
    if (rc == URF_OK)
        rc = order_after_slots(c);   /* the staging arrays are shared with the callback path */
    if (rc != URF_OK)
        return rc;
    if (n_total)
        hipLaunchKernelGGL(k_pc2_to_soa, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, c->stream, d_data,
                           (unsigned long long)n_total, point_step, off_x, off_y, off_z, c->sx.p, c->sy.p, c->sz.p);
    return classify_batch(c, URF_LAST_PC2, urf_call{ c->sx.p, c->sy.p, c->sz.p, d_offsets, n_per_scan, max_len, n_scans, d_labels, d_info });
}

extern "C" int urf_classify_batch_pc2(urf_ctx* c, const uint8_t* d_data, uint32_t n_per_scan, uint32_t n_scans,
                                      uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                      uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c || !d_data || !pc2_layout_ok(point_step, off_x, off_y, off_z))
        return URF_ERR_INVALID_ARG;
    if (n_scans > c->max_batch || n_per_scan > c->max_points)
        return URF_ERR_CAPACITY;
    return classify_batch_pc2(c, d_data, nullptr, (uint64_t)n_per_scan * n_scans, n_per_scan, n_per_scan, n_scans, point_step, off_x, off_y,
                              off_z, d_labels, d_info);
}

/* A zero-length scan of a ragged batch is one the pipeline already answers with URF_TOO_FEW_POINTS (urf_classify_batch_soa_ragged
 * does the same). */
extern "C" int urf_classify_batch_pc2_ragged(urf_ctx* c, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total,
                                             uint32_t max_len, uint32_t n_scans, uint32_t point_step, uint32_t off_x,
                                             uint32_t off_y, uint32_t off_z, uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c || !d_data || !d_offsets || !d_labels || !pc2_layout_ok(point_step, off_x, off_y, off_z))
        return URF_ERR_INVALID_ARG;
    if (n_scans > c->max_batch || max_len > c->max_points || n_total > (uint64_t)c->max_points * c->max_batch)
        return URF_ERR_CAPACITY;
    return classify_batch_pc2(c, d_data, d_offsets, n_total, 0, max_len, n_scans, point_step, off_x, off_y, off_z, d_labels, d_info);
}

/* ---- dense sweeps: put back into firing slots by laser id, then the pipeline (urf_k_dense.hpp) ------------------------------- */
extern "C" int urf_set_dense_slots(urf_ctx* c, const uint8_t* slot_of_id, uint32_t n_ids)
{
    if (!c || n_ids > 256u)
        return URF_ERR_INVALID_ARG;
    for (unsigned i = 0; i < 256u; i++)   /* (a copy; the device gets it with the next dense call, outside every captured sequence) */
        c->dense_map[i] = !slot_of_id ? (uint8_t)i : i < n_ids ? slot_of_id[i] : (uint8_t)0xff;
    c->dense_map_dirty = true;
    return URF_OK;
}

/* the per-scan words of a dense call inside dn_words: per-tile counts and bases, the aligned flags, the call's aligned count */
static uint32_t* dense_word(urf_ctx* c, int which)
{
    const size_t per_tile = (size_t)c->max_batch * c->max_tiles;
    return c->dn_words.p + (which == 0 ? 0 : which == 1 ? per_tile : which == 2 ? 2 * per_tile : 2 * per_tile + c->max_batch);
}

extern "C" int urf_dense_scans(urf_ctx* c, uint32_t* n_aligned)
{
    if (!c || !n_aligned)
        return URF_ERR_INVALID_ARG;
    *n_aligned = 0;
    if (!c->dn_words.p)   /* (no dense call yet) */
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));
    URF_HIP(c, hipMemcpy(n_aligned, dense_word(c, 3), sizeof(uint32_t), hipMemcpyDeviceToHost));
    return URF_OK;
}

/* d: where ids and points come from (id*, x / y / z or data and its layout; the rest is filled in here).  The padded batch -- n_scans
 * scans of W * L points in the SoA staging, NaN wherever no point landed -- is a plain batch call to everything behind the scatter. */
static int classify_batch_dense(urf_ctx* c, int kind, urf_dense_args d, const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info, bool elev = false)
{
    const uint64_t WL = (uint64_t)max_firings * (uint32_t)c->params.channels;
    if (WL > c->max_points || max_len > WL || n_scans > c->max_batch)
        return URF_ERR_CAPACITY;
    if (n_scans == 0)
        return URF_OK;
    if (max_firings == 0)   /* (and max_len == 0: a padded scan of no points is no batch call) */
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    const size_t n_all = (size_t)c->max_points * c->max_batch, per_tile = (size_t)c->max_batch * c->max_tiles;
    int rc;
    if ((rc = ensure_soa_staging(c)) != URF_OK || (rc = grow(c, c->dn_pos, n_all)) != URF_OK || (rc = grow(c, c->dn_labels, n_all)) != URF_OK ||
        (rc = grow(c, c->dn_words, 2 * per_tile + c->max_batch + 1)) != URF_OK || (rc = grow(c, c->dn_map, 256)) != URF_OK)
        return rc;
    if (elev && ((rc = grow(c, c->dn_ids, n_all)) != URF_OK || (rc = grow(c, c->dn_elev, 1)) != URF_OK))
        return rc;
    if ((rc = order_after_slots(c)) != URF_OK)   /* the staging arrays are shared with the callback path */
        return rc;
    hipStream_t st = c->stream;
    if (c->dense_map_dirty) {   /* (rare: behind whatever still reads the old map) */
        URF_HIP(c, hipStreamSynchronize(st));
        URF_HIP(c, hipMemcpy(c->dn_map.p, c->dense_map, sizeof(c->dense_map), hipMemcpyHostToDevice));
        c->dense_map_dirty = false;
    }
    if (elev && c->dense_elev_dirty) {   /* (as rare, and as far outside every captured sequence) */
        URF_HIP(c, hipStreamSynchronize(st));
        URF_HIP(c, hipMemcpy(c->dn_elev.p, &c->dense_elev, sizeof(c->dense_elev), hipMemcpyHostToDevice));
        c->dense_elev_dirty = false;
    }
    d.offsets = d_offsets;
    d.max_len = max_len;
    d.n_scans = n_scans;
    d.tiles = (max_len + URF_TILE - 1) / URF_TILE;
    if (d.tiles == 0)
        d.tiles = 1;
    d.L = (uint32_t)c->params.channels;
    d.W = max_firings;
    d.slot_of_id = c->dn_map.p;
    if (elev) {   /* derived ids are slots already: the table's identity, not urf_set_dense_slots' map */
        d.id = c->dn_ids.p;
        d.id_stride = d.id_bytes = 1u;
        d.slot_of_id = c->dn_elev.p->identity;
    }
    d.tile_cnt = dense_word(c, 0);
    d.tile_base = dense_word(c, 1);
    d.aligned = dense_word(c, 2);
    d.n_aligned = dense_word(c, 3);
    d.px = c->sx.p;
    d.py = c->sy.p;
    d.pz = c->sz.p;
    d.pos = c->dn_pos.p;
    d.padded_labels = c->dn_labels.p;
    d.labels = d_labels;
    /* the holes are NaN: the call's range of the staging as all-ones bytes, every call (a shorter batch must not see an earlier one's points) */
    const size_t fill = (size_t)n_scans * (size_t)WL * sizeof(float);
    URF_HIP(c, hipMemsetAsync(c->sx.p, 0xff, fill, st));
    URF_HIP(c, hipMemsetAsync(c->sy.p, 0xff, fill, st));
    URF_HIP(c, hipMemsetAsync(c->sz.p, 0xff, fill, st));
    URF_HIP(c, hipMemsetAsync(d.n_aligned, 0, sizeof(uint32_t), st));
    const dim3 g_tiles(d.tiles, n_scans);
    if (elev) {
        const urf_dense_ids_args e{ c->dn_elev.p, c->dn_ids.p, (unsigned long long)c->dn_ids.cap };
        if (kind == URF_LAST_PC2)
            hipLaunchKernelGGL(k_dense_ids_pc2, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d, e);
        else
            hipLaunchKernelGGL(k_dense_ids_soa, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d, e);
        c->dn_ids_call.d = d;
        c->dn_ids_call.e = e;
        c->dn_ids_call.kind = (uint32_t)kind;
    }
    hipLaunchKernelGGL(k_dense_count, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d);
    hipLaunchKernelGGL(k_dense_scan, dim3(n_scans), dim3(URF_DENSE_THREADS), 0, st, d);
    if (kind == URF_LAST_PC2)
        hipLaunchKernelGGL(k_dense_scatter_pc2, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d);
    else
        hipLaunchKernelGGL(k_dense_scatter_soa, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d);
    URF_HIP(c, hipGetLastError());
    rc = classify_batch(c, kind, urf_call{ c->sx.p, c->sy.p, c->sz.p, nullptr, (uint32_t)WL, (uint32_t)WL, n_scans, c->dn_labels.p, d_info });
    if (rc != URF_OK)
        return rc;
    hipLaunchKernelGGL(k_dense_labels, g_tiles, dim3(URF_DENSE_THREADS), 0, st, d);
    URF_HIP(c, hipGetLastError());
    /* the record of the last call: the padded batch (all buffers the context's), marked dense, with what urf_clouds_batch_* in input
     * order read -- the caller's labels and inputs, the offsets as the context's copy (the padded call has none of its own) */
    URF_HIP(c, hipMemcpyAsync(c->offsets_copy, d_offsets, ((size_t)n_scans + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    c->last.dense.on = true;
    c->last.dense.x = d.x;
    c->last.dense.y = d.y;
    c->last.dense.z = d.z;
    c->last.dense.labels = d_labels;
    c->last.dense.max_len = max_len;
    c->dn_calls++;   /* (dn_pos is another call's now: dn_inv holds no inverse of it) */
    return URF_OK;
}

extern "C" int urf_set_dense_outputs(urf_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1))
        return URF_ERR_INVALID_ARG;
    c->dense_outputs = on != 0;   /* (dn_inv grows with the first read-out that needs it: dense_unmap) */
    return URF_OK;
}

extern "C" int urf_classify_batch_soa_dense(urf_ctx* c, const float* d_x, const float* d_y, const float* d_z, const void* d_laser,
                                            uint32_t laser_bytes, const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                            uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c || !d_x || !d_y || !d_z || !d_laser || !d_offsets || !d_labels || (laser_bytes != 1u && laser_bytes != 2u))
        return URF_ERR_INVALID_ARG;
    urf_dense_args d{};
    d.id = (const uint8_t*)d_laser;
    d.id_stride = laser_bytes;
    d.id_bytes = laser_bytes;
    d.x = d_x;
    d.y = d_y;
    d.z = d_z;
    return classify_batch_dense(c, URF_LAST_SOA, d, d_offsets, max_len, n_scans, max_firings, d_labels, d_info);
}

/* ---- ... by ids derived from the points' elevation: clouds without a `ring` field ------------------------------- */
extern "C" int urf_set_dense_elevations(urf_ctx* c, const float* elev_deg, uint32_t n)
{
    if (!c || (!elev_deg && n != 0) || (elev_deg && (n == 0 || n > URF_DENSE_ELEV_MAX)))
        return URF_ERR_INVALID_ARG;
    for (uint32_t l = 0; l < n; l++)
        if (!(elev_deg[l] > -90.f && elev_deg[l] < 90.f))   /* (NaN fails both) */
            return URF_ERR_INVALID_ARG;
    /* slots by ascending elevation, the lower slot first among equals; thresholds at the tangents of the midpoints, in double */
    uint8_t rank_slot[URF_DENSE_ELEV_MAX];
    for (uint32_t l = 0; l < n; l++)
        rank_slot[l] = (uint8_t)l;
    std::stable_sort(rank_slot, rank_slot + n, [&](uint8_t a, uint8_t b) { return elev_deg[a] < elev_deg[b]; });
    urf_dense_elev_table& t = c->dense_elev;
    for (uint32_t k = 0; k < URF_DENSE_ELEV_MAX; k++) {
        t.thr[k] = INFINITY;
        t.slot_of_rank[k] = k < n ? rank_slot[k] : (uint8_t)0xff;
        if (k + 1 < n)
            t.thr[k] = (float)std::tan(((double)elev_deg[rank_slot[k]] + (double)elev_deg[rank_slot[k + 1]]) / 2.0 * 3.14159265358979323846 / 180.0);
    }
    c->dense_elev_n = n;
    c->dense_elev_dirty = true;   /* (a copy; the device gets it with the next elevation call) */
    return URF_OK;
}

/* the refusal the elevation calls add to the dense calls' */
static bool refuse_elev(urf_ctx* c, const char* what)
{
    if (c->dense_elev_n != 0 && c->dense_elev_n == (uint32_t)c->params.channels)
        return false;
    c->last_error = std::string(what) + (c->dense_elev_n == 0 ? ": no elevation table (urf_set_dense_elevations)"
                                                               : ": the elevation table's size is not the parameters' channels");
    return true;
}

extern "C" int urf_classify_batch_soa_dense_elev(urf_ctx* c, const float* d_x, const float* d_y, const float* d_z, const uint32_t* d_offsets,
                                                 uint32_t max_len, uint32_t n_scans, uint32_t max_firings, uint8_t* d_labels,
                                                 urf_scan_info* d_info)
{
    if (!c || !d_x || !d_y || !d_z || !d_offsets || !d_labels || refuse_elev(c, "urf_classify_batch_soa_dense_elev"))
        return URF_ERR_INVALID_ARG;
    urf_dense_args d{};
    d.x = d_x;
    d.y = d_y;
    d.z = d_z;
    return classify_batch_dense(c, URF_LAST_SOA, d, d_offsets, max_len, n_scans, max_firings, d_labels, d_info, true);
}

extern "C" int urf_classify_batch_pc2_dense_elev(urf_ctx* c, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total,
                                                 uint32_t max_len, uint32_t n_scans, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                                                 uint32_t off_z, uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info)
{
    if (!c || !d_data || !d_offsets || !d_labels || !pc2_layout_ok(point_step, off_x, off_y, off_z) ||
        refuse_elev(c, "urf_classify_batch_pc2_dense_elev"))
        return URF_ERR_INVALID_ARG;
    if (n_total > (uint64_t)c->max_points * c->max_batch)
        return URF_ERR_CAPACITY;
    urf_dense_args d{};
    d.data = d_data;
    d.step = point_step;
    d.ox = off_x;
    d.oy = off_y;
    d.oz = off_z;
    return classify_batch_dense(c, URF_LAST_PC2, d, d_offsets, max_len, n_scans, max_firings, d_labels, d_info, true);
}

extern "C" int urf_classify_batch_pc2_dense(urf_ctx* c, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total, uint32_t max_len,
                                            uint32_t n_scans, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                            uint32_t off_laser, uint32_t laser_bytes, uint32_t max_firings, uint8_t* d_labels,
                                            urf_scan_info* d_info)
{
    if (!c || !d_data || !d_offsets || !d_labels || !pc2_layout_ok(point_step, off_x, off_y, off_z) || (laser_bytes != 1u && laser_bytes != 2u) ||
        (uint64_t)off_laser + laser_bytes > point_step)
        return URF_ERR_INVALID_ARG;
    if (n_total > (uint64_t)c->max_points * c->max_batch)
        return URF_ERR_CAPACITY;
    urf_dense_args d{};
    d.id = d_data + off_laser;
    d.id_stride = point_step;
    d.id_bytes = laser_bytes;
    d.data = d_data;
    d.step = point_step;
    d.ox = off_x;
    d.oy = off_y;
    d.oz = off_z;
    return classify_batch_dense(c, URF_LAST_PC2, d, d_offsets, max_len, n_scans, max_firings, d_labels, d_info);
}

/* ---- the read-out chain: published order and marker points of scans [s0, s0 + n) of a run ------------------------------- */
struct urf_readout_dst {
    uint32_t *road, *curb, *r10, stride, *lcounts;
    float* pts;
    uint32_t* mcount;
};

/* The one launch sequence of the read-out kernels, results to d: a sweep of the callback path behind its pipeline (sweep_outputs_launch:
 * s0 = 0, n = 1, captured with the sweep) and the batch read-backs on the context's stream (readouts_of_last).  products: URF_SWEEP_OUT_ORDER | URF_SWEEP_OUT_MARKER_POINTS; prep: the pre-pass of a fused run's read-outs is to
 * be launched; merged (both products, n == 1): the per-ring work of the two products is one launch (k_sweep_rings), lists and marker
 * points another (k_sweep_lists); direct (n == 1): the last kernels store to d's mapped host memory themselves, the lists back to back.
 * One linear chain on `st`, separate launches as the only synchronisation.  A fused run (r.a.front) holds the *_front siblings on the
 * grids of the general kernels, in the order of the captured sequences: ring, ring_front, literal, literal_front.  Every general
 * read-out kernel returns at once for a scan where urf_scan_fused holds and every *_front kernel where it does not (urf_k_outputs.hpp,
 * urf_k_front_outputs.hpp): a scan is served by exactly one of each pair, so the order among them changes no result. */
static int launch_readouts(urf_ctx* c, const urf_run& r, hipStream_t st, uint32_t s0, uint32_t n, const urf_readout_view& v, uint32_t products,
                           bool prep, bool merged, bool direct, const urf_readout_dst& d)
{
    const urf_kargs& a = r.a;
    const urf_dev_params& dp = r.dp;
    const bool mark = (products & URF_SWEEP_OUT_MARKER_POINTS) != 0, order = (products & URF_SWEEP_OUT_ORDER) != 0, fused = a.front != 0;
    uint8_t* const mk_lit = v.mk_red + n * (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;   /* one flag per ring and scan behind the cells */
    const dim3 g_ring((unsigned)dp.p.channels, n), g_lists((unsigned)dp.p.channels + 1u, n), b256(256);
    const size_t map_lds = (2 * (size_t)a.tiles + 1) * sizeof(unsigned);
    if (prep)
        hipLaunchKernelGGL(k_front_out_prep, dim3(a.tiles, n), b256, 0, st, a, dp, s0, v.fo_az, v.fo_ent, v.fo_d);
    if (merged) {
        hipLaunchKernelGGL(k_sweep_rings, g_ring, b256, map_lds, st, a, dp, urf_ring_outs{ v.ord_keys, v.ord_pos, v.ord_cls, v.mk_d, v.mk_pos, v.mk_red, mk_lit });
    } else {
        if (order)
            hipLaunchKernelGGL(k_ring_order, g_ring, b256, map_lds, st, a, dp, s0, v.ord_keys, v.ord_pos, v.ord_cls);
        if (mark)
            hipLaunchKernelGGL(k_marker_ring, g_ring, b256, map_lds, st, a, dp, s0, v.mk_d, v.mk_pos, v.mk_red, mk_lit);
    }
    if (fused && order)
        hipLaunchKernelGGL(k_ring_order_front, g_ring, b256, 0, st, a, dp, s0, v.fo_az, v.fo_ent, v.ord_pos, v.ord_cls);
    if (fused && mark)
        hipLaunchKernelGGL(k_marker_ring_front, g_ring, b256, 0, st, a, dp, s0, v.fo_az, v.fo_ent, v.fo_d, v.mk_d, v.mk_pos, v.mk_red, mk_lit);
    if (mark) {   /* rings in which the ORDER of equal azimuths decides a marker point (normally none: every workgroup returns at once) */
        hipLaunchKernelGGL(k_marker_ring_literal, g_ring, b256, 0, st, a, dp, s0, mk_lit, v.mk_d, v.mk_pos, v.mk_red);
        if (fused)
            hipLaunchKernelGGL(k_marker_ring_literal_front, g_ring, b256, 0, st, a, dp, s0, mk_lit, v.fo_az, v.fo_ent, v.fo_d, v.mk_d, v.mk_pos, v.mk_red);
    }
    if (merged) {
        if (direct)
            hipLaunchKernelGGL(k_sweep_lists_direct, g_lists, dim3(384), 0, st, a, dp,
                               urf_sweep_lists_args{ v.ord_pos, v.ord_cls, d.road, nullptr, nullptr, d.lcounts, 0u, v.mk_d, v.mk_pos, v.mk_red, d.pts, d.mcount });
        else
            hipLaunchKernelGGL(k_sweep_lists, g_lists, dim3(384), 0, st, a, dp,
                               urf_sweep_lists_args{ v.ord_pos, v.ord_cls, d.road, d.curb, d.r10, d.lcounts, d.stride, v.mk_d, v.mk_pos, v.mk_red, d.pts, d.mcount });
    } else {
        if (order && direct)
            hipLaunchKernelGGL(k_ordered_lists_direct, g_ring, b256, 0, st, a, dp, v.ord_pos, v.ord_cls, d.road, d.lcounts);
        else if (order)
            hipLaunchKernelGGL(k_ordered_lists, g_ring, b256, 0, st, a, dp, s0, v.ord_pos, v.ord_cls, d.road, d.curb, d.r10, d.stride, d.lcounts);
        if (mark) {
            hipLaunchKernelGGL(k_marker_bins, dim3(n), dim3(384), 0, st, a, dp, s0, v.mk_d, v.mk_pos, v.mk_red, d.pts, d.mcount);
            if (fused)
                hipLaunchKernelGGL(k_marker_bins_front, dim3(n), dim3(384), 0, st, a, dp, s0, v.mk_d, v.mk_pos, v.mk_red, d.pts, d.mcount);
        }
    }
    URF_HIP(c, hipGetLastError());
    return URF_OK;
}

#include "urf_api_sweep.hpp"

/* Step 1 of last_call(), on its own for the entry points that check sizes of theirs against the call before any HIP call: a last call
 * exists, holds `scan` (a batch read-out: 0) and is of `kind` where that matters (urf_clouds_batch_*).  nullptr: URF_ERR_INVALID_ARG. */
static const urf_last_call* last_valid(urf_ctx* c, uint32_t scan = 0, int kind = URF_LAST_NONE)
{
    const urf_last_call& l = c->last;
    if (kind != URF_LAST_NONE && l.kind != kind) {
        c->last_error = l.kind == URF_LAST_SOA || l.kind == URF_LAST_PC2 ? "the last batch call was of the other kind (SoA / PointCloud2)"
                                                                         : "the last classify call was no batch call (urf_classify_batch_*)";
        return nullptr;
    }
    return scan < l.scans && l.run.a.labels ? &l : nullptr;   /* (no call yet: no scans) */
}

/* After a dense call (urf_classify_batch_*_dense) the record is the PADDED batch: what answers in padded indices -- urf_ordered_indices*,
 * urf_clouds_batch_* in the reference order, urf_read_stage -- is refused, unless it is one of the lists (`mapped`) and
 * urf_set_dense_outputs is on: launch_ordered then maps them back to the caller's indices (dense_unmap). */
static bool refuse_dense(urf_ctx* c, const char* what, bool mapped = false)
{
    if (!c->last.dense.on || (mapped && c->dense_outputs))
        return false;
    c->last_error = std::string(what) + ": not available after a dense call (urf_classify_batch_*_dense): its results index the padded sweeps";
    return true;
}

/* The readers' way to the last call and its scratch ROW: valid, on the context's device, the row intact and ring-sorted, the context's
 * stream behind the sweeps in flight.  A sweep's row is only intact while no later sweep has been submitted on it (slots that share a
 * row: max_batch < URF_MAX_IN_FLIGHT and more sweeps in flight than rows). */
enum urf_last_need { URF_NEED_RING_SORTED, URF_NEED_RING_ORDER };   /* the row's ring-sorted copies (urf_read_stage) | the rings' points in order, from either path */
static int last_call(urf_ctx* c, uint32_t scan, const urf_last_call*& out, urf_last_need need)
{
    urf_last_call& l = c->last;
    if (!(out = last_valid(c, scan)))
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    if (l.kind == URF_LAST_SWEEP && c->row_gen[l.row] != l.gen) {
        c->last_error = "the scratch row of the sweep waited for last has been resubmitted (create the context with max_batch >= "
                        "the number of sweeps in flight, or read its intermediate results before submitting on its row again)";
        return URF_ERR_BUSY;
    }
    int rc = URF_OK;
    if (l.run.a.front && !(need == URF_NEED_RING_ORDER && c->pol.front_outputs)) {
        /* the last call went through the fused front end (urf_front.hpp), which keeps no ring-sorted copies: once more on its row through
         * the general kernels, as a batch call with every repair kernel in the sequence (same inputs -- a batch caller's arrays must still
         * be alive, a sweep of the callback path is still in its slot's device buffer and its row has not been resubmitted (checked
         * above) --, same parameters, same labels), and the context stays with them: a caller that reads ring-sorted results pays for
         * them once, not per call.  Only the record's run changes: a sweep stays the sweep it was (row, gen, sweep_n, dense).
         * With urf_set_front_outputs on, the entry points that only need the rings' points in order (URF_NEED_RING_ORDER) take the fused
         * call as it is: launch_ordered / launch_markers run the kernels of urf_k_front_outputs.hpp next to the general ones. */
        c->pol.set(c->pol.want_ring_sorted, true);
        const urf_kargs& a = l.run.a;
        rc = run_pipeline(c, urf_call{ a.x, a.y, a.z, a.offsets, a.n_per_scan, a.max_len, a.n_scans, a.labels, nullptr, l.row, nullptr, &l.run.dp,
                                       (int)a.capture, true }, l.run);
        c->last_seq++;
    }
    return rc != URF_OK ? rc : order_after_slots(c);
}

/* ---- urf_front_explain (include/urf.h) ------------------------------------------------------ */
/* The last call's record without last_call()'s second run: the function reads what the call left behind -- front_ok, front_ncand, the
 * summaries, the final ring tables -- and the call's own points, launches k_front_explain on the context's stream and touches nothing a
 * classify call reads (no want_ring_sorted, no epoch, no flag word). */
extern "C" int urf_front_explain(urf_ctx* c, int layout, urf_front_why* out, uint32_t n)
{
    if (c && !out && n == 0 && (layout == 0 || layout == 1))   /* (the adapters' question: how many records) */
        return last_valid(c) ? (int)c->last.scans : 0;
    const urf_last_call* lp = c ? last_valid(c) : nullptr;
    if (!lp || !out || (layout != 0 && layout != 1) || n != lp->scans)
        return URF_ERR_INVALID_ARG;
    const urf_last_call& l = *lp;
    URF_HIP(c, hipSetDevice(c->device));
    if (l.kind == URF_LAST_SWEEP && c->row_gen[l.row] != l.gen) {
        c->last_error = "urf_front_explain: the scratch row of the sweep waited for last has been resubmitted";
        return URF_ERR_BUSY;
    }
    int rc = grow(c, c->fx_rec, (size_t)n * URF_FX_WORDS, c->stream);
    if (rc != URF_OK || (rc = order_after_slots(c)) != URF_OK)
        return rc;
    const urf_kargs& a = l.run.a;
    const urf_dev_params& dp = l.run.dp;
    const unsigned L = (unsigned)dp.p.channels;
    const bool rows = layout == 1 && !l.dense.on;   /* (a dense call: the padded batch, firing order) */
    const bool lasers = L == 16u || L == 32u || L == 64u || L == 128u;   /* (other counts: no laser slots to speak of, the counters stay 0) */
    hipStream_t st = c->stream;
    std::vector<uint32_t> rec((size_t)n * URF_FX_WORDS, 0u), ok(n), ncand(n), lens(n, l.sweep_n ? l.sweep_n : a.n_per_scan);
    std::vector<urf_scan_info> info(n);
    if (lasers) {
        URF_HIP(c, hipMemsetAsync(c->fx_rec.p, 0, rec.size() * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_front_explain, dim3(a.tiles, n), dim3(64), 0, st, a, dp, rows ? 1u : 0u, c->fx_rec.p);
        URF_HIP(c, hipGetLastError());
        URF_HIP(c, hipMemcpyAsync(rec.data(), c->fx_rec.p, rec.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    URF_HIP(c, hipMemcpyAsync(ok.data(), a.front_ok, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    URF_HIP(c, hipMemcpyAsync(ncand.data(), a.front_ncand, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    URF_HIP(c, hipMemcpyAsync(info.data(), a.info, n * sizeof(urf_scan_info), hipMemcpyDeviceToHost, st));
    if (a.offsets) {
        std::vector<uint32_t> offs((size_t)n + 1);
        URF_HIP(c, hipMemcpyAsync(offs.data(), a.offsets, offs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        URF_HIP(c, hipStreamSynchronize(st));
        for (uint32_t s = 0; s < n; s++)
            lens[s] = std::min(offs[s + 1] - offs[s], a.max_len);
    }
    URF_HIP(c, hipStreamSynchronize(st));
    const urf_fx_call k = fx_call_of(l.run, rows, 0u);
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t* r = &rec[(size_t)s * URF_FX_WORDS];
        const urf_fx_scan v = urf_front_scan_rule(k, r, ok[s], ncand[s], info[s].status, lens[s]);   /* (the rule k_front_digest applies on the device) */
        urf_front_why w;
        std::memset(&w, 0, sizeof w);
        w.fused = v.fused;
        w.call = l.run.planned.call.why;
        w.advice = l.run.planned.call.advice | v.advice;
        w.scan = v.scan;
        w.candidates = ncand[s];
        w.candidate_cap = a.front_cand_cap;
        if (info[s].status == URF_OK && lens[s] != 0u) {
            w.lanes_two_rings = urf_fx_bits4(r + URF_FX_LANE_MASK);
            w.rings_two_lanes = urf_fx_bits4(r + URF_FX_RING_MASK);
            w.axis_points = r[URF_FX_AXIS];
            w.range_points = r[URF_FX_RANGE];
            w.multi_sector_firings = r[URF_FX_MULTI];
            w.max_sectors_per_firing = r[URF_FX_MAX_SECTORS];
            w.tiles_sectors_fall = r[URF_FX_FALL];
        }
        out[s] = w;
    }
    return URF_OK;
}

/* ---- index-set and marker outputs: every scan of a batch in one launch sequence ------------- */
extern "C" int urf_compact_indices_batch(urf_ctx* c, const uint8_t* d_labels, uint32_t n_per_scan, uint32_t n_scans,
                                         uint32_t* d_road, uint32_t* d_curb, uint32_t* d_roi, uint32_t* d_ring10,
                                         uint32_t* d_counts)
{
    if (!c || !d_labels)
        return URF_ERR_INVALID_ARG;
    if (n_scans > c->max_batch || n_per_scan > c->max_points)
        return URF_ERR_CAPACITY;
    if (n_scans == 0 || n_per_scan == 0)
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    {
        const int orc = order_after_slots(c);   /* compact_cnt is shared scratch */
        if (orc != URF_OK)
            return orc;
    }
    const unsigned tiles = (n_per_scan + URF_TILE - 1) / URF_TILE;
    const dim3 grid(tiles, n_scans);
    hipLaunchKernelGGL(k_compact_count, grid, dim3(URF_COMPACT_THREADS), 0, c->stream, d_labels, n_per_scan, tiles, c->compact_cnt);
    hipLaunchKernelGGL(k_compact_write, grid, dim3(URF_COMPACT_THREADS), 0, c->stream, d_labels, n_per_scan, tiles, c->compact_cnt,
                       d_road, d_curb, d_roi, d_ring10, d_counts);
    URF_HIP(c, hipGetLastError());
    return URF_OK;
}

extern "C" int urf_compact_indices(urf_ctx* c, const uint8_t* d_labels, uint32_t n_points,
                                   uint32_t* d_road, uint32_t* d_curb, uint32_t* d_roi, uint32_t* d_ring10,
                                   uint32_t* d_counts)
{
    return urf_compact_indices_batch(c, d_labels, n_points, 1, d_road, d_curb, d_roi, d_ring10, d_counts);
}

/* The read-out chain for scans [s0, s0 + n) of the last classify call (l: from last_call) on the context's stream: the scratch of the
 * wanted products grown to n scans, for a fused record (last_call: only with urf_set_front_outputs on) the pre-pass's too; then
 * launch_readouts, with the pre-pass unless its arrays already hold exactly that (same recorded call, same range). */
static int readouts_of_last(urf_ctx* c, const urf_last_call& l, uint32_t s0, uint32_t n, uint32_t products, const urf_readout_dst& d)
{
    urf_readout_scratch& w = c->ro;
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS, ss = (size_t)n * c->sstride;
    hipStream_t st = c->stream;
    int rc = URF_OK;
    if ((products & URF_SWEEP_OUT_ORDER) && ((rc = grow(c, w.ord_keys, ss, st)) != URF_OK || (rc = grow(c, w.ord_pos, ss, st)) != URF_OK ||
                                             (rc = grow(c, w.ord_cls, (size_t)n * URF_MAX_CHANNELS * 2, st)) != URF_OK))
        return rc;
    if ((products & URF_SWEEP_OUT_MARKER_POINTS) && ((rc = grow(c, w.mk_d, n * cells, st)) != URF_OK || (rc = grow(c, w.mk_pos, n * cells, st)) != URF_OK ||
                                                     (rc = grow(c, w.mk_red, n * (cells + URF_MAX_CHANNELS), st)) != URF_OK))
        return rc;
    bool prep = false;
    if (l.run.a.front) {
        prep = ss > w.fo_az.cap || ss > w.fo_ent.cap || ss > w.fo_d.cap || c->fo_prep.seq != c->last_seq || c->fo_prep.s0 != s0 || c->fo_prep.n != n;
        if (prep)
            c->fo_prep.seq = 0;
        if ((rc = grow(c, w.fo_az, ss, st)) != URF_OK || (rc = grow(c, w.fo_ent, ss, st)) != URF_OK || (rc = grow(c, w.fo_d, ss, st)) != URF_OK)
            return rc;
    }
    if ((rc = launch_readouts(c, l.run, st, s0, n, w.view(0, c->sstride), products, prep, false, false, d)) == URF_OK && prep)
        c->fo_prep = { c->last_seq, s0, n };   /* (the mark only behind a launch that was accepted) */
    return rc;
}

/* The lists k_ordered_lists wrote for scans [s0, s0 + n) of a dense call, from padded positions to the caller's dense indices, in place
 * (urf_k_dense.hpp).  The inverse of dn_pos is built by the first read-out behind a dense call and kept for the others. */
static int dense_unmap(urf_ctx* c, const urf_last_call& l, uint32_t s0, uint32_t n, uint32_t* d_road, uint32_t* d_curb, uint32_t* d_r10,
                       uint32_t stride, const uint32_t* d_counts)
{
    hipStream_t st = c->stream;
    const bool regrow = (size_t)c->max_points * c->max_batch > c->dn_inv.cap;
    if (regrow)
        c->dn_inv_of = 0;
    const int rc = grow(c, c->dn_inv, (size_t)c->max_points * c->max_batch, st);
    if (rc != URF_OK)
        return rc;
    const uint32_t WL = l.run.a.max_len, max_len = l.dense.max_len;   /* (the padded call's scans are W * L points each) */
    urf_dense_unmap_args u{ c->offsets_copy, max_len, WL, c->dn_pos.p, c->dn_inv.p };
    if (c->dn_inv_of != c->dn_calls) {
        c->dn_inv_of = 0;
        const unsigned tiles = max_len ? (max_len + URF_TILE - 1) / URF_TILE : 1u;
        hipLaunchKernelGGL(k_dense_inverse, dim3(tiles, l.scans), dim3(URF_DENSE_THREADS), 0, st, u);
        URF_HIP(c, hipGetLastError());   /* (the mark only behind a launch that was accepted) */
        c->dn_inv_of = c->dn_calls;
    }
    const uint32_t most = stride < max_len ? stride : max_len;   /* (a list holds points of the scan: at most its length) */
    hipLaunchKernelGGL(k_dense_unmap_lists, dim3(most ? (most + URF_DENSE_THREADS - 1) / URF_DENSE_THREADS : 1u, n, 3), dim3(URF_DENSE_THREADS), 0,
                       st, u, s0, d_road, d_curb, d_r10, stride, d_counts);
    URF_HIP(c, hipGetLastError());
    return URF_OK;
}

/* scans [s0, s0 + n) of the last classify call (l: from last_call), lists of `stride` entries per scan on the device */
static int launch_ordered(urf_ctx* c, const urf_last_call& l, uint32_t s0, uint32_t n, uint32_t* d_road, uint32_t* d_curb, uint32_t* d_r10,
                          uint32_t stride, uint32_t* d_counts)
{
    const int rc = readouts_of_last(c, l, s0, n, URF_SWEEP_OUT_ORDER, urf_readout_dst{ d_road, d_curb, d_r10, stride, d_counts, nullptr, nullptr });
    if (rc != URF_OK)
        return rc;
    return l.dense.on ? dense_unmap(c, l, s0, n, d_road, d_curb, d_r10, stride, d_counts) : URF_OK;   /* (refuse_dense: the switch is on) */
}

extern "C" int urf_ordered_indices_batch(urf_ctx* c, uint32_t* d_road, uint32_t* d_curb, uint32_t* d_ring10, uint32_t stride,
                                         uint32_t* d_counts)
{
    const urf_last_call* l = c ? last_valid(c) : nullptr;
    if (!l || !d_counts || refuse_dense(c, "urf_ordered_indices_batch", true) || stride < (l->dense.on ? l->dense.max_len : l->run.a.max_len))
        return URF_ERR_INVALID_ARG;   /* (a dense call's lists hold dense points: none is longer than its max_len) */
    const int rc = last_call(c, 0, l, URF_NEED_RING_ORDER);
    return rc != URF_OK ? rc : launch_ordered(c, *l, 0, l->scans, d_road, d_curb, d_ring10, stride, d_counts);
}

extern "C" int urf_ordered_indices(urf_ctx* c, uint32_t scan, uint32_t* road, uint32_t* curb, uint32_t* ring10,
                                   uint32_t* counts)
{
    if (!c || !counts || refuse_dense(c, "urf_ordered_indices", true))
        return URF_ERR_INVALID_ARG;
    const size_t mp = c->sstride;
    const urf_last_call* l;
    int rc;
    if ((rc = last_call(c, scan, l, URF_NEED_RING_ORDER)) != URF_OK || (rc = grow(c, c->ord_lists, mp * 3 + 4)) != URF_OK)
        return rc;
    uint32_t* d_road = c->ord_lists.p;
    uint32_t* d_curb = d_road + mp;
    uint32_t* d_r10 = d_curb + mp;
    uint32_t* d_cnt = d_r10 + mp;
    hipStream_t st = c->stream;
    if ((rc = launch_ordered(c, *l, scan, 1, d_road, d_curb, d_r10, (uint32_t)mp, d_cnt)) != URF_OK)
        return rc;
    uint32_t h[3] = { 0, 0, 0 };
    URF_HIP(c, hipMemcpyAsync(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    URF_HIP(c, hipStreamSynchronize(st));
    if (road && h[0])
        URF_HIP(c, hipMemcpy(road, d_road, h[0] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (curb && h[1])
        URF_HIP(c, hipMemcpy(curb, d_curb, h[1] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ring10 && h[2])
        URF_HIP(c, hipMemcpy(ring10, d_r10, h[2] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    counts[0] = h[0];
    counts[1] = h[1];
    counts[2] = h[2];
    return URF_OK;
}

/* ---- the published clouds of a batch (urf_k_clouds.hpp) ---------------------------------------------- */
#define URF_DBG_CLOUDS_NT 16u   /* test hook (urf_set_debug_flags): the records go out with non-temporal stores (A/B, tools/batch_clouds_bench.py) */

static int ensure_clouds_scratch(urf_ctx* c, uint32_t n_scans, uint32_t stride, bool lists)
{
    const int rc = grow(c, c->cl_tiles, 2 * (size_t)c->max_batch * c->max_tiles);
    if (rc != URF_OK || !lists)
        return rc;
    return grow(c, c->cl_lists, 3 * (size_t)n_scans * stride + 3 * (size_t)n_scans, c->stream);
}

/* src: where the points come from (x / y / z / data and the layout fields; the rest is filled in here) */
static int clouds_batch(urf_ctx* c, int kind, urf_clouds_args src, int order, urf_point_xyzi* d_records, uint64_t capacity,
                        uint32_t* d_counts, uint64_t* d_offsets)
{
    const urf_last_call* l;
    if (!d_counts || !d_offsets || (order != URF_ORDER_INPUT && order != URF_ORDER_REFERENCE) || !(l = last_valid(c, 0, kind)))
        return URF_ERR_INVALID_ARG;
    /* a dense call: the caller's dense labels, inputs and offsets; the reference order is the padded batch's, mapped back by launch_ordered
     * under urf_set_dense_outputs */
    const bool dense = l->dense.on;
    if (dense && order == URF_ORDER_REFERENCE && refuse_dense(c, "urf_clouds_batch_* with URF_ORDER_REFERENCE", true))
        return URF_ERR_INVALID_ARG;
    const uint32_t S = l->scans, max_len = dense ? l->dense.max_len : l->run.a.max_len, stride = max_len ? max_len : 1u;
    if (d_records && capacity < 3ull * S * max_len)
        return URF_ERR_CAPACITY;
    URF_HIP(c, hipSetDevice(c->device));
    const bool ref = order == URF_ORDER_REFERENCE && d_records;
    int rc = ensure_clouds_scratch(c, S, stride, ref);
    if (rc != URF_OK)
        return rc;
    if (ref) {   /* urf_ordered_indices_batch's kernels (after a fused call: the documented rerun through the general kernels) */
        uint32_t* const o = c->cl_lists.p;
        if ((rc = last_call(c, 0, l, URF_NEED_RING_ORDER)) == URF_OK)
            rc = launch_ordered(c, *l, 0, S, o, o + (size_t)S * stride, o + 2 * (size_t)S * stride, stride, o + 3 * (size_t)S * stride);
    } else {
        rc = order_after_slots(c);   /* cl_tiles is the context's; the input order needs nothing ring-sorted of the row */
    }
    if (rc != URF_OK)
        return rc;
    const urf_kargs& a = l->run.a;   /* (after a rerun: the same labels, inputs and offsets) */
    src.labels = a.labels;
    src.offsets = a.offsets;
    src.info = a.info;
    src.n_per_scan = a.n_per_scan;
    src.max_len = a.max_len;
    src.tiles = a.tiles;
    if (dense) {
        src.labels = l->dense.labels;
        src.offsets = c->offsets_copy;
        src.n_per_scan = 0;
        src.max_len = max_len;
        src.tiles = max_len ? (max_len + URF_TILE - 1) / URF_TILE : 1u;
        if (kind == URF_LAST_SOA) {
            src.x = (const unsigned*)l->dense.x;
            src.y = (const unsigned*)l->dense.y;
            src.z = (const unsigned*)l->dense.z;
        }
    }
    src.n_scans = S;
    src.tile_cnt = c->cl_tiles.p;
    src.tile_base = src.tile_cnt + (size_t)c->max_batch * c->max_tiles;
    src.counts = d_counts;
    src.offs = (unsigned long long*)d_offsets;
    src.rec = (urf_u32x4*)d_records;
    src.lists = c->cl_lists.p;
    src.list_cnt = c->cl_lists.p ? c->cl_lists.p + 3 * (size_t)S * stride : nullptr;
    src.stride = stride;
    hipStream_t st = c->stream;
    const dim3 g_tiles(src.tiles, S);
    hipLaunchKernelGGL(k_clouds_count, g_tiles, dim3(URF_CLOUDS_COUNT_THREADS), 0, st, src);
    hipLaunchKernelGGL(k_clouds_scan, dim3(S), dim3(URF_CLOUDS_THREADS), 0, st, src);
    hipLaunchKernelGGL(k_clouds_offsets, dim3(1), dim3(URF_CLOUDS_OFF_THREADS), 0, st, src);
    if (d_records) {
        const bool nt = (c->debug_flags & URF_DBG_CLOUDS_NT) != 0;
        const unsigned which = ref ? 0x4u : 0xfu;
        if (nt)
            hipLaunchKernelGGL(k_clouds_write<true>, g_tiles, dim3(URF_CLOUDS_THREADS), 0, st, src, which);
        else
            hipLaunchKernelGGL(k_clouds_write<false>, g_tiles, dim3(URF_CLOUDS_THREADS), 0, st, src, which);
        if (ref) {
            const dim3 g_list((stride + URF_CLOUDS_THREADS - 1) / URF_CLOUDS_THREADS, S, 3);
            if (nt)
                hipLaunchKernelGGL(k_clouds_gather<true>, g_list, dim3(URF_CLOUDS_THREADS), 0, st, src);
            else
                hipLaunchKernelGGL(k_clouds_gather<false>, g_list, dim3(URF_CLOUDS_THREADS), 0, st, src);
        }
    }
    URF_HIP(c, hipGetLastError());
    return URF_OK;
}

extern "C" int urf_clouds_batch_soa(urf_ctx* c, const float* d_intensity, int order, urf_point_xyzi* d_records, uint64_t capacity,
                                    uint32_t* d_counts, uint64_t* d_offsets)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    urf_clouds_args src{};
    src.src = URF_SRC_SOA;
    src.x = (const unsigned*)c->last.run.a.x;
    src.y = (const unsigned*)c->last.run.a.y;
    src.z = (const unsigned*)c->last.run.a.z;
    src.in = (const unsigned*)d_intensity;
    src.oi = -1;
    return clouds_batch(c, URF_LAST_SOA, src, order, d_records, capacity, d_counts, d_offsets);
}

extern "C" int urf_clouds_batch_pc2(urf_ctx* c, const uint8_t* d_data, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                                    uint32_t off_z, int32_t off_intensity, int order, urf_point_xyzi* d_records, uint64_t capacity,
                                    uint32_t* d_counts, uint64_t* d_offsets)
{
    if (!c || !d_data || !pc2_layout_ok(point_step, off_x, off_y, off_z) || off_intensity < -1 ||
        (off_intensity >= 0 && (uint64_t)off_intensity + 4 > point_step))
        return URF_ERR_INVALID_ARG;
    urf_clouds_args src{};
    src.data = d_data;
    src.step = point_step;
    src.ox = off_x;
    src.oy = off_y;
    src.oz = off_z;
    src.oi = off_intensity;
    const uint32_t oi = off_intensity >= 0 ? (uint32_t)off_intensity : 0u;
    if (((uintptr_t)d_data | point_step) % 16 == 0 && off_x == 0 && off_y == 4 && off_z == 8 && oi % 4 == 0)
        src.src = URF_SRC_PC2_XYZ;   /* pcl::PointXYZI, PointXYZ + intensity (Velodyne), Ouster records */
    else if (((uintptr_t)d_data | point_step | off_x | off_y | off_z | oi) % 4 == 0)
        src.src = URF_SRC_PC2;
    else
        src.src = URF_SRC_PC2_BYTES;
    return clouds_batch(c, URF_LAST_PC2, src, order, d_records, capacity, d_counts, d_offsets);
}

static int launch_markers(urf_ctx* c, const urf_last_call& l, uint32_t s0, uint32_t n, float* d_pts, uint32_t* d_counts)
{
    return readouts_of_last(c, l, s0, n, URF_SWEEP_OUT_MARKER_POINTS, urf_readout_dst{ nullptr, nullptr, nullptr, 0u, nullptr, d_pts, d_counts });
}

extern "C" int urf_marker_points_batch(urf_ctx* c, float* d_pts, uint32_t* d_counts)
{
    if (!c || !d_pts || !d_counts)
        return URF_ERR_INVALID_ARG;
    const urf_last_call* l;
    const int rc = last_call(c, 0, l, URF_NEED_RING_ORDER);
    return rc != URF_OK ? rc : launch_markers(c, *l, 0, l->scans, d_pts, d_counts);
}

extern "C" int urf_marker_points(urf_ctx* c, uint32_t scan, float* pts, uint32_t* count)
{
    if (!c || !pts || !count)
        return URF_ERR_INVALID_ARG;
    const urf_last_call* l;
    int rc;
    if ((rc = last_call(c, scan, l, URF_NEED_RING_ORDER)) != URF_OK || (rc = grow(c, c->mk_out, URF_DEG_CELLS * 4 + 4)) != URF_OK)
        return rc;
    hipStream_t st = c->stream;
    unsigned* d_cnt = (unsigned*)(c->mk_out.p + URF_DEG_CELLS * 4);
    if ((rc = launch_markers(c, *l, scan, 1, c->mk_out.p, d_cnt)) != URF_OK)
        return rc;
    std::vector<float> h(URF_DEG_CELLS * 4 + 4);
    URF_HIP(c, hipMemcpyAsync(h.data(), c->mk_out.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    URF_HIP(c, hipStreamSynchronize(st));
    uint32_t n = 0;
    std::memcpy(&n, &h[URF_DEG_CELLS * 4], sizeof(n));
    if (n > URF_DEG_CELLS)
        return URF_ERR_HIP;
    std::memcpy(pts, h.data(), (size_t)n * 4 * sizeof(float));
    *count = n;
    return URF_OK;
}

/* road_marker's line strips for n_scans sets of marker points (include/urf.h).  Reads nothing of the context but its stream:
 * no scratch row, nothing of the last classify call. */
extern "C" int urf_marker_strips_batch(urf_ctx* c, const urf_marker_params* mp, const float* d_pts, const uint32_t* d_counts, uint32_t n_scans,
                                       int sequence, int32_t* d_ghost, urf_marker_strip* d_strips, float* d_xyz, uint32_t* d_n)
{
    if (!c || !mp || mp->size != sizeof(urf_marker_params) || !d_pts || !d_counts || !d_strips || !d_xyz || !d_n)
        return URF_ERR_INVALID_ARG;
    if (n_scans > c->max_batch)
        return URF_ERR_CAPACITY;
    if (n_scans == 0)
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    const int32_t* ghost_in = nullptr;
    if (sequence && d_ghost) {   /* a copy: scan 0's wave may read it after the last scan's wave has written the new value */
        int rc = grow(c, c->mk_ghost, 1);
        if (rc != URF_OK)
            return rc;
        URF_HIP(c, hipMemcpyAsync(c->mk_ghost.p, d_ghost, sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        ghost_in = c->mk_ghost.p;
    }
    hipLaunchKernelGGL(k_marker_strips, dim3(n_scans), dim3(URF_WAVE), 0, c->stream, d_pts, d_counts, n_scans, sequence ? 1 : 0, *mp, ghost_in,
                       sequence ? d_ghost : nullptr, d_strips, d_xyz, d_n);
    URF_HIP(c, hipGetLastError());
    return URF_OK;
}

/* ---- stage-wise inspection -------------------------------------------------- */
template <class T>
static int fetch(urf_ctx* c, std::vector<T>& dst, const T* src, size_t count)
{
    dst.resize(count);
    if (count)
        URF_HIP(c, hipMemcpy(dst.data(), src, count * sizeof(T), hipMemcpyDeviceToHost));
    return URF_OK;
}

/* The ring-sorted slots of scan `scan` that hold a point (index relative to the scan's scratch
 * base) and the input index of each, rebuilt on the host from k_split's per-tile tables: tile t
 * fills its first troff[t][C] slots. */
static int ring_slot_sources(urf_ctx* c, const urf_last_call& l, uint32_t scan, uint32_t len, std::vector<uint32_t>& slot, std::vector<uint32_t>& src)
{
    const urf_kargs& k = l.run.a;
    const unsigned C = (unsigned)l.run.dp.p.channels;
    const unsigned ntiles = (len + URF_TILE - 1) / URF_TILE;
    std::vector<uint16_t> troff;
    std::vector<uint32_t> rec;
    int rc;
    if ((rc = fetch(c, troff, k.troff + (size_t)scan * k.tiles * (C + 1), (size_t)ntiles * (C + 1))) != URF_OK) return rc;
    if ((rc = fetch(c, rec, k.rec + (size_t)scan * k.sstride, (size_t)ntiles * URF_TILE)) != URF_OK) return rc;
    slot.clear();
    src.clear();
    for (unsigned t = 0; t < ntiles; t++)
        for (unsigned j = 0; j < troff[(size_t)t * (C + 1) + C]; j++) {
            slot.push_back(t * URF_TILE + j);
            src.push_back(t * URF_TILE + (rec[(size_t)t * URF_TILE + j] & URF_REC_SRC_MASK));
        }
    return URF_OK;
}

extern "C" int urf_read_stage(urf_ctx* c, urf_stage what, uint32_t scan, void* host_dst, size_t bytes)
{
    if (!c || !host_dst || refuse_dense(c, "urf_read_stage"))
        return URF_ERR_INVALID_ARG;
    const urf_last_call* l;
    int rc = last_call(c, scan, l, URF_NEED_RING_SORTED);   /* (stage values are the general kernels', whatever urf_set_front_outputs says) */
    if (rc != URF_OK)
        return rc;
    URF_HIP(c, hipStreamSynchronize(c->stream));
    const urf_kargs& k = l->run.a;   /* the arguments and parameters of the call whose results are read */
    uint32_t len;
    if (k.offsets) {
        uint32_t o2[2];
        URF_HIP(c, hipMemcpy(o2, k.offsets + scan, sizeof(o2), hipMemcpyDeviceToHost));
        len = o2[1] - o2[0];
        if (len > k.max_len)
            len = k.max_len;
    } else {
        len = l->sweep_n ? l->sweep_n : k.n_per_scan;   /* (a padded sweep: the caller's points) */
    }
    const unsigned C = (unsigned)l->run.dp.p.channels;
    const size_t sb = (size_t)scan * k.sstride;
    urf_scan_info in;
    URF_HIP(c, hipMemcpy(&in, k.info + scan, sizeof(in), hipMemcpyDeviceToHost));
    switch (what) {
    case URF_STAGE_VALPHA:
        if (k.capture != 1) return URF_ERR_INVALID_ARG;
        if (bytes < len * sizeof(float)) return URF_ERR_INVALID_ARG;
        URF_HIP(c, hipMemcpy(host_dst, k.valpha + sb, len * sizeof(float), hipMemcpyDeviceToHost));
        return URF_OK;
    case URF_STAGE_RING: {
        if (k.capture == 0) return URF_ERR_INVALID_ARG;
        if (bytes < len * sizeof(int16_t)) return URF_ERR_INVALID_ARG;
        std::vector<uint8_t> rk;
        if ((rc = fetch(c, rk, k.ringkey + sb, len)) != URF_OK) return rc;
        int16_t* o = (int16_t*)host_dst;
        for (uint32_t i = 0; i < len; i++)
            o[i] = (in.status != URF_OK || rk[i] == URF_RING_NONE) ? (int16_t)-1 : (int16_t)rk[i];
        return URF_OK;
    }
    case URF_STAGE_SECTOR: {
        if (k.capture == 0) return URF_ERR_INVALID_ARG;
        if (bytes < len * sizeof(int16_t)) return URF_ERR_INVALID_ARG;
        std::vector<uint16_t> sk;
        if ((rc = fetch(c, sk, k.seckey + sb, len)) != URF_OK) return rc;
        int16_t* o = (int16_t*)host_dst;
        for (uint32_t i = 0; i < len; i++)
            o[i] = sk[i] == URF_SEC_NONE ? (int16_t)-1 : (int16_t)sk[i];
        return URF_OK;
    }
    case URF_STAGE_AZIMUTH:
    case URF_STAGE_RANGE2D:
    case URF_STAGE_DETECT: {
        if (what != URF_STAGE_DETECT && k.capture != 1) return URF_ERR_INVALID_ARG;   /* exact values need the capture */
        const size_t esz = what == URF_STAGE_DETECT ? 1 : 4;
        if (bytes < len * esz) return URF_ERR_INVALID_ARG;
        std::memset(host_dst, 0, len * esz);
        if (in.status != URF_OK) return URF_OK;
        std::vector<uint32_t> slot, src;
        if ((rc = ring_slot_sources(c, *l, scan, len, slot, src)) != URF_OK) return rc;
        const size_t span = (size_t)((len + URF_TILE - 1) / URF_TILE) * URF_TILE;
        if (what == URF_STAGE_DETECT) {
            std::vector<uint32_t> rec;   /* the detector hits of a slot's record */
            if ((rc = fetch(c, rec, k.rec + sb, span)) != URF_OK) return rc;
            uint8_t* o = (uint8_t*)host_dst;
            for (size_t p = 0; p < slot.size(); p++)
                o[src[p]] = (uint8_t)((rec[slot[p]] >> URF_REC_FLAG_SHIFT) & 7u);
        } else {
            std::vector<float> v;
            if ((rc = fetch(c, v, (what == URF_STAGE_AZIMUTH ? k.caz : k.rd2) + sb, span)) != URF_OK) return rc;
            float* o = (float*)host_dst;
            for (size_t p = 0; p < slot.size(); p++)
                o[src[p]] = v[slot[p]];
        }
        return URF_OK;
    }
    case URF_STAGE_ANGLE_TABLE: {
        if (bytes < C * sizeof(float)) return URF_ERR_INVALID_ARG;
        std::memset(host_dst, 0, C * sizeof(float));
        if (in.status != URF_OK) return URF_OK;
        URF_HIP(c, hipMemcpy(host_dst, k.angle + (size_t)scan * C, in.n_rings * sizeof(float), hipMemcpyDeviceToHost));
        return URF_OK;
    }
    case URF_STAGE_MAXDIST: {
        if (bytes < C * sizeof(float)) return URF_ERR_INVALID_ARG;
        std::memset(host_dst, 0, C * sizeof(float));
        if (in.status != URF_OK) return URF_OK;
        URF_HIP(c, hipMemcpy(host_dst, k.maxdist + (size_t)scan * C, in.n_rings * sizeof(float), hipMemcpyDeviceToHost));
        return URF_OK;
    }
    case URF_STAGE_QUADRANTS:
        if (bytes < 4 * sizeof(float)) return URF_ERR_INVALID_ARG;
        URF_HIP(c, hipMemcpy(host_dst, k.quad + (size_t)scan * 4, 4 * sizeof(float), hipMemcpyDeviceToHost));
        return URF_OK;
    case URF_STAGE_BEAM_STOP:
        if (bytes < 2 * URF_DEG_CELLS * sizeof(int16_t)) return URF_ERR_INVALID_ARG;
        URF_HIP(c, hipMemcpy(host_dst, k.stop_f + (size_t)scan * URF_DEG_CELLS, URF_DEG_CELLS * sizeof(int16_t), hipMemcpyDeviceToHost));
        URF_HIP(c, hipMemcpy((int16_t*)host_dst + URF_DEG_CELLS, k.stop_b + (size_t)scan * URF_DEG_CELLS,
                             URF_DEG_CELLS * sizeof(int16_t), hipMemcpyDeviceToHost));
        return URF_OK;
    }
    return URF_ERR_INVALID_ARG;
}

/* ---- test and benchmark hooks (include/urf_test_hooks.h) --------------------------------------------
 * Compiled only into liburf_hip_test.so (-DURF_ENABLE_TEST_HOOKS, urban_road_filter_amd/build.py): the product
 * library liburf_hip.so exports none of them. */
#ifdef URF_ENABLE_TEST_HOOKS
extern "C" int urf_set_debug_flags(urf_ctx* c, uint32_t flags)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    c->debug_flags = flags;
    c->dp.exp_flags = flags;
    c->pol.epoch++;
    return URF_OK;
}

extern "C" int urf_selftest(urf_ctx* c, uint64_t* n_mismatches)
{
    if (!c || !n_mismatches)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    URF_HIP(c, hipMalloc((void**)&d, sizeof(*d)));
    URF_HIP(c, hipMemsetAsync(d, 0, sizeof(*d), c->stream));
    hipLaunchKernelGGL(k_selftest_div_pi, dim3(c->n_cus * 8), dim3(256), 0, c->stream, d);
    unsigned long long h = 0;
    hipError_t e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    URF_HIP(c, e);
    *n_mismatches = h;
    return URF_OK;
}

extern "C" int urf_selftest_fast(urf_ctx* c, uint64_t n_samples, float* err)
{
    if (!c || !err)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    unsigned* d = nullptr;
    URF_HIP(c, hipMalloc((void**)&d, 4 * sizeof(unsigned)));
    URF_HIP(c, hipMemsetAsync(d, 0, 4 * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(k_selftest_fast, dim3(c->n_cus * 8), dim3(256), 0, c->stream, (unsigned long long)n_samples, c->dp.Kfi, d);
    hipError_t e = hipMemcpyAsync(err, d, 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    URF_HIP(c, e);
    return URF_OK;
}

/* the first n bytes of dn_ids as the last elevation call left them */
extern "C" int urf_test_dense_ids(urf_ctx* c, uint8_t* host, uint64_t n)
{
    if (!c || !host || n > c->dn_ids.cap)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));
    if (n)
        URF_HIP(c, hipMemcpy(host, c->dn_ids.p, n, hipMemcpyDeviceToHost));
    return URF_OK;
}

/* the id kernel of the last elevation call launched `reps` times again between two events: *ms = the mean of one launch */
extern "C" int urf_test_dense_ids_ms(urf_ctx* c, uint32_t reps, float* ms)
{
    if (!c || !ms || reps == 0 || c->dn_ids_call.kind == URF_LAST_NONE)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    URF_HIP(c, hipEventCreate(&e0));
    hipError_t err = hipEventCreate(&e1);
    if (err == hipSuccess) {
        const urf_dense_args& d = c->dn_ids_call.d;
        const dim3 g_tiles(d.tiles, d.n_scans);
        (void)hipEventRecord(e0, c->stream);
        for (uint32_t r = 0; r < reps; r++) {
            if (c->dn_ids_call.kind == URF_LAST_PC2)
                hipLaunchKernelGGL(k_dense_ids_pc2, g_tiles, dim3(URF_DENSE_THREADS), 0, c->stream, d, c->dn_ids_call.e);
            else
                hipLaunchKernelGGL(k_dense_ids_soa, g_tiles, dim3(URF_DENSE_THREADS), 0, c->stream, d, c->dn_ids_call.e);
        }
        (void)hipEventRecord(e1, c->stream);
        err = hipEventSynchronize(e1);
        if (err == hipSuccess)
            err = hipEventElapsedTime(ms, e0, e1);
        (void)hipEventDestroy(e1);
    }
    (void)hipEventDestroy(e0);
    URF_HIP(c, err);
    *ms /= (float)reps;
    return URF_OK;
}

#endif   /* URF_ENABLE_TEST_HOOKS */

