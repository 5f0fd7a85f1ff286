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

#define URF_ASYNC_SLOTS 4
static_assert(URF_ASYNC_SLOTS == URF_MAX_IN_FLIGHT, "include/urf.h documents the number of sweeps in flight");

/* A lazily sized buffer of T -- device memory, or pinned host memory (Host) --: grow() makes it large enough for the largest
 * request so far, and the context frees it with itself. */
template <class T, bool Host = false>
struct lazy_buf {
    T* p = nullptr;
    size_t cap = 0;   /* elements */
    lazy_buf() = default;
    lazy_buf(const lazy_buf&) = delete;
    lazy_buf& operator=(const lazy_buf&) = delete;
    ~lazy_buf() { release(); }
    void release()
    {
        if (p)
            (void)(Host ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
/* Pinned host memory that kernels write themselves (urf_set_sweep_results_direct): mapped into the device's address space and coherent,
 * so that the host sees the stores once the event behind the kernel has completed, whatever the environment says about host memory. */
struct mapped_buf {
    uint32_t* p = nullptr;    /* the host's pointer */
    uint32_t* dev = nullptr;  /* the device's (hipHostGetDevicePointer) */
    size_t cap = 0;           /* words */
    mapped_buf() = default;
    mapped_buf(const mapped_buf&) = delete;
    mapped_buf& operator=(const mapped_buf&) = delete;
    ~mapped_buf() { release(); }
    void release()
    {
        if (p)
            (void)hipHostFree(p);
        p = dev = nullptr;
        cap = 0;
    }
};

/* Every scratch array of urf_kargs, declared once with its elements per row: X(field, elements).  A row is one scan's slice of
 * each array -- scan r of a batch call, or the sweep of the callback path that runs on row r -- and starts r * elements into it
 * (kargs_row).  Most arrays have max_batch rows; the two per-call counters (SLOTS: the URF_LIST_COUNT work-list lengths and the
 * ring-count hint) have URF_ASYNC_SLOTS, one per sweep in flight, whatever max_batch is.  urf_create allocates SCANS and SLOTS;
 * CAPTURE comes with the first urf_enable_stage_capture, ROW_MAJOR (the firing-order copies of row-major organised sweeps) once
 * such a sweep has been sighted (rows_state_update), LASERS128 (what the fused front end sizes for 64 lanes, sized for 128: urf_front.hpp)
 * with the first urf_set_front_lasers128(ctx, 1), MULTI_SECTOR (the star records' sectors, k_front*_ms -> k_front_sectors) with the first
 * urf_set_front_multi_sector(ctx, 1).  sstride, max_tiles and front_cand_cap are the context's (scratch_walk). */
#define URF_SCRATCH_SCANS(X)                                                                                                     \
    X(rx, sstride) X(ry, sstride) X(rz, sstride) X(rec, sstride)                                                                 \
    X(sr, sstride) X(sz, sstride) X(sslot, sstride) X(ssrt16, sstride) X(ssrt, sstride) X(wsg, sstride)                          \
    X(big_r, sstride) X(big_z, sstride) X(big_i, sstride)                                                                        \
    X(tile_roi, max_tiles) X(roi_bits, max_tiles * (URF_TILE / 64)) X(troff, max_tiles * (URF_MAX_CHANNELS + 1))                 \
    X(tsoff, max_tiles * (URF_MAX_SECTORS + 1)) X(tmaxs, max_tiles * URF_MAX_CHANNELS)                                           \
    X(rpre, URF_MAX_CHANNELS * (max_tiles + 1)) X(rstart, URF_MAX_CHANNELS * max_tiles)                                          \
    X(angle, URF_MAX_CHANNELS) X(ring_thr, URF_MAX_CHANNELS * 4) X(ring_lut, URF_LUT_CELLS) X(ring_cnt, URF_MAX_CHANNELS)        \
    X(ring_off, URF_MAX_CHANNELS + 1)                                                                                            \
    X(sec_cnt, URF_MAX_SECTORS) X(sec_run, URF_MAX_SECTORS) X(sec_off, URF_MAX_SECTORS + 1) X(star_hit, URF_MAX_SECTORS)         \
    X(star_first, URF_MAX_SECTORS) X(star_list_mid, URF_MAX_SECTORS) X(star_list_big, URF_MAX_SECTORS)                           \
    X(star_list_runs, URF_MAX_SECTORS) X(tie_list, URF_MAX_SECTORS) X(tie_post, URF_MAX_SECTORS)                                 \
    X(table_upto, 1) X(table_redo, 1) X(redo_list, 1) X(table_cause, 1)                                                          \
    X(nan_mask, 4) X(nan_list, 2 * URF_MAX_CHANNELS) X(vis, URF_MAX_CHANNELS)                                                    \
    X(maxdist, URF_MAX_CHANNELS) X(quad, 4)                                                                                      \
    X(curb_cnt, URF_MAX_CHANNELS) X(curb_az, URF_MAX_CHANNELS * URF_CURB_LIST)                                                   \
    X(sufmin, URF_MAX_CHANNELS * URF_DEG_CELLS) X(premax, URF_MAX_CHANNELS * URF_DEG_CELLS)                                      \
    X(stop_f, URF_DEG_CELLS) X(stop_b, URF_DEG_CELLS)                                                                            \
    X(win, URF_MAX_CHANNELS * URF_DEG_CELLS)                                                                                     \
    X(info, 1)                                                                                                                   \
    X(front_ok, 1) X(front_pres, max_tiles * 64) X(front_maxs, max_tiles * 64) X(front_lane_ring, 64)                            \
    X(front_ring_lane, URF_MAX_CHANNELS) X(front_cand, front_cand_cap) X(front_all, front_cand_cap) X(front_ncand, 1)             \
    X(front_list, 1) X(front_st, URF_FRONT_ST_WORDS)
#define URF_SCRATCH_SLOTS(X) X(list_len, URF_LIST_COUNT) X(ring_hint, 1)
#define URF_SCRATCH_CAPTURE(X) X(valpha, sstride) X(seckey, sstride) X(ringkey, sstride) X(rd2, sstride) X(caz, sstride)
#define URF_SCRATCH_ROW_MAJOR(X) X(tx, sstride) X(ty, sstride) X(tz, sstride) X(rows_v, 64) X(rows_ok, 1)
#define URF_SCRATCH_LASERS128(X)                                                                                                  \
    X(front_pres128, URF_FRONT128_TILES2(max_tiles) * 64) X(front_maxs128, URF_FRONT128_TILES2(max_tiles) * 64)                  \
    X(front_lane_ring128, URF_FRONT128_L) X(front_st128, URF_FRONT128_ST_WORDS) X(rows_v128, URF_FRONT128_L)                     \
    X(front_cand128, URF_FRONT128_CAND_CAP(max_points)) X(front_all128, URF_FRONT128_CAND_CAP(max_points))
#define URF_SCRATCH_MULTI_SECTOR(X) X(front_skey, sstride)
enum urf_scratch_group { URF_SCR_ALWAYS, URF_SCR_CAPTURE, URF_SCR_ROW_MAJOR, URF_SCR_LASERS128, URF_SCR_MULTI_SECTOR };

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

/* "The last call", for the entry points that take their input from it (urf_read_stage, urf_ordered_indices, urf_marker_points,
 * urf_clouds_batch_*): publish_last() is the only writer of the whole record, last_call() the readers' way to it. */
enum urf_last_kind { URF_LAST_NONE, URF_LAST_SOA, URF_LAST_PC2, URF_LAST_SWEEP };   /* no call yet | the batch entry point | a sweep waited for */
/* plan()'s decision about a call in words, kept for urf_front_explain: the terms that were false and the advice (urf_policy::why), and
 * whether the march was, or would have been, the multi-sector one (ms_ok) */
struct urf_planned {
    urf_policy::reasons call = { 0u, 0u };
    bool ms = false;
};
/* the call's part of the per-scan rule (urf_front_scan_rule): `rows`, the layout the records are counted in; sweep_n, a sweep's own length */
static urf_fx_call fx_call_of(const urf_kargs& a, const urf_dev_params& dp, const urf_planned& planned, bool rows, uint32_t sweep_n)
{
    const uint32_t L = (uint32_t)dp.p.channels;
    return urf_fx_call{ a.front, a.front_rows, a.front_cand_cap, rows ? 1u : 0u, (L == 16u || L == 32u || L == 64u || L == 128u) ? L : 0u,
                        planned.ms ? 1u : 0u, dp.p.curbPoints != 5 ? 1u : 0u, planned.call.why, sweep_n };
}
struct urf_last_call {
    int kind = URF_LAST_NONE;
    uint32_t scans = 0;
    urf_kargs a;                    /* the kernel arguments and parameters it ran with */
    urf_dev_params dp;
    uint32_t row = 0;               /* the scratch row of a.* (a batch call: 0) */
    uint64_t gen = 0;               /* a sweep: the row's submission number it was (urf_ctx::row_gen) */
    urf_planned planned;            /* what the policy said about the call when it planned it (urf_front_explain) */
    uint32_t sweep_n = 0;           /* a sweep: the caller's number of points (urf_set_sweep_quantum: a.n_per_scan is the padded length) */
    /* a dense call (urf_classify_batch_*_dense): `a` is the padded batch -- staging, padded labels, all the context's own --, and
     * this is what the caller handed in, for urf_clouds_batch_* in input order (offsets: the context's copy) */
    struct {
        bool on = false;
        const float *x = nullptr, *y = nullptr, *z = nullptr;   /* a SoA call's */
        uint8_t* labels = nullptr;
        uint32_t max_len = 0;
    } dense;
};

struct urf_ctx {
    int device = 0;
    uint32_t max_points = 0, max_batch = 0;
    uint32_t max_tiles = 0;
    uint32_t sstride = 0;           /* scratch elements per scan: max_tiles * URF_TILE + URF_SCAN_PAD */
    uint32_t debug_flags = 0;       /* urf_set_debug_flags */
    unsigned n_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    urf_params params;
    urf_dev_params dp;
    urf_kargs k;                    /* device pointers (context-owned part): the scratch arrays (URF_SCRATCH_*) at row 0 */
    /* owned device memory of fixed size: the scratch arrays and the tables, freed by urf_destroy */
    std::vector<void*> allocs;
    lazy_buf<float> sx, sy, sz;     /* SoA staging for PointCloud2 input: max_batch x max_points */
    /* The single-scan (callback) path: URF_ASYNC_SLOTS sweeps in flight, so that -- with a context created
     * for several scans -- the copies and kernels of several sweeps overlap on the device (a single sweep's
     * kernels are a few dozen workgroups each).  Per slot: pinned host staging for the message bytes and for the
     * results, device copies of both, the captured launch sequence. */
    struct slot_t {
        lazy_buf<uint8_t, true> h_in;   /* the largest message so far */
        lazy_buf<uint8_t> d_raw;        /* ... its device copy */
        lazy_buf<uint8_t, true> h_labels;   /* max_points */
        lazy_buf<uint8_t> d_labels;     /* max_points */
        lazy_buf<urf_scan_info, true> h_info;
        hipEvent_t ev_done = nullptr;
        /* the captured launch sequences: one, or with urf_set_sweep_quantum up to URF_SWEEP_SEQS, one per padded length (seq_find) */
        struct seq_t {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            uint64_t key[3] = { 0, 0, 0 };  /* what the captured sequence was built for */
            urf_kargs cap_a;                /* ... and the kernel arguments / parameters it runs with */
            urf_dev_params cap_dp;
            urf_planned cap_planned;        /* ... and what the policy said when it planned them */
            uint64_t used = 0;              /* urf_ctx::seq_clock of its last launch: the least recently used one makes room */
        } seqs[URF_SWEEP_SEQS];
        urf_kargs cap_a;                /* the arguments / parameters / plan of the sweep in this slot (its sequence's, or its direct launches') */
        urf_dev_params cap_dp;
        urf_planned cap_planned;
        bool pending = false, used = false;
        uint64_t gen = 0;               /* the row's submission number of the sweep in this slot */
        uint32_t n_points = 0, ticket = 0;
        /* urf_set_sweep_quantum: the points the sweep runs as (n_points rounded up to the quantum, NaN behind the caller's; off: n_points),
         * whether its sequence is a padded one, and the sweep's own length for k_pc2_to_soa_pad: a pinned word and its device copy */
        uint32_t n_run = 0;
        bool pad = false;
        lazy_buf<uint32_t, true> h_n;
        lazy_buf<uint32_t> d_n;
        uint32_t point_step = 0, off_x = 0, off_y = 0, off_z = 0;   /* layout of the message in d_raw */
        bool planes = false;            /* d_raw holds x[n] y[n] z[n] (a staged message) instead of the records */
        /* urf_set_sweep_outputs: the sweep's marker points and ordered lists (sweep_out_words: URF_SWEEP_HDR words, then three
         * lists of n_points entries), device and pinned; out_bits: the bits the sweep in this slot was submitted with */
        lazy_buf<uint32_t> d_out;
        lazy_buf<uint32_t, true> h_out;
        uint32_t out_bits = 0;
        /* urf_set_sweep_results_direct: the same products stored by the kernels themselves (URF_SWEEP_HDR words, then the three lists back
         * to back: at most 2 x max_points entries -- road and curb are disjoint sets of the sweep's points, ring 10 has at most all of them);
         * out_direct: whether the sweep in this slot was submitted that way, i.e. which buffer and which list layout its results have */
        mapped_buf m_out;
        bool out_direct = false;
    } slots[URF_ASYNC_SLOTS];
    /* urf_set_sweep_outputs: what launch_markers / launch_ordered / front_out_prepare keep as context-wide lazy buffers, once per scratch
     * row of the callback path (row r starts r * elements into each: sweep_row) -- a sweep's captured sequence produces its read-outs on
     * its own row.  Allocated by the first call that turns a bit on; empty in a context that never does. */
    struct sweep_scratch_t {
        lazy_buf<float> mk_d;               /* [rows][URF_MAX_CHANNELS * URF_DEG_CELLS] */
        lazy_buf<uint32_t> mk_pos;
        lazy_buf<uint8_t> mk_red;           /* ... + URF_MAX_CHANNELS literal flags (mk_lit) behind the cells of a row */
        lazy_buf<unsigned long long> ord_keys;   /* [rows][sstride] */
        lazy_buf<uint32_t> ord_pos;
        lazy_buf<uint32_t> ord_cls;         /* [rows][URF_MAX_CHANNELS * 2] */
        lazy_buf<uint32_t> fo_az, fo_ent;   /* [rows][sstride] */
        lazy_buf<float> fo_d;
    } sweep;
    bool streams_made = false;
    urf_policy pol;                 /* which kernels a call launches */
    uint32_t n_rerun = 0;           /* sweeps urf_classify_pc2_wait had to run again */
    uint32_t n_captured = 0;        /* launch sequences captured so far, all slots (urf_callback_path_captures) */
    uint64_t seq_clock = 0;         /* launches of captured sequences so far (slot_t::seq_t::used) */
    /* Slot i works on scratch row i % rows, rows = min(max_batch, URF_ASYNC_SLOTS); row 0 runs on the
     * context's stream, every other row on a stream of its own (slots that share a row share its
     * stream: they are serialised).  Everything else the context launches runs on `stream`; the two
     * kinds of work are ordered against each other by events (order_after_slots / order_row_after_main). */
    hipStream_t row_stream[URF_ASYNC_SLOTS] = { nullptr, nullptr, nullptr, nullptr };
    hipEvent_t ev_main = nullptr;          /* recorded on `stream` for a row stream to wait on */
    uint64_t main_seq = 1;                 /* bumped by every launch on `stream` that touches scratch rows >= 1 or the staging */
    uint64_t row_seen[URF_ASYNC_SLOTS] = { 0, 0, 0, 0 };
    /* Slots that share a scratch row (max_batch < URF_ASYNC_SLOTS) are serialised on the row's stream, and a later
     * sweep overwrites the row.  Labels and summary of every sweep are safe (each slot has its own result buffers,
     * filled in stream order); what reads the ROW afterwards (urf_read_stage / urf_ordered_indices /
     * urf_marker_points) checks that the sweep published as "the last call" is still the row's latest submission (last_call). */
    uint64_t row_gen[URF_ASYNC_SLOTS] = { 0, 0, 0, 0 };   /* submissions on the row so far */
    uint32_t next_ticket = 0;
    /* sized for the largest number of scans asked for so far: scratch of the index-list and marker-point outputs
     * (sstride entries resp. channels x 361 cells per scan) */
    lazy_buf<unsigned long long> ord_keys;
    lazy_buf<uint32_t> ord_pos;
    lazy_buf<uint32_t> ord_cls;     /* [scans][URF_MAX_CHANNELS][2] road / curb points per ring (k_ring_order -> k_ordered_lists) */
    lazy_buf<uint32_t> ord_lists;   /* single-scan entry point: 3 x sstride + 4 */
    /* the read-outs of a fused call (urf_k_front_outputs.hpp): [scans][sstride] per ring-major position the exact azimuth's bits, the entry
     * input index | class << 30 and the planar distance.  k_front_out_prep fills them once per recorded call and range of scans (fo_prep:
     * the call's number and the range they hold; nobody writes them afterwards), for urf_ordered_indices* and urf_marker_points* alike. */
    lazy_buf<uint32_t> fo_az, fo_ent;
    lazy_buf<float> fo_d;
    struct { uint64_t seq = 0; uint32_t s0 = 0, n = 0; } fo_prep;
    uint64_t last_seq = 0;          /* bumped whenever `last` is written */
    lazy_buf<float> mk_d;
    lazy_buf<uint32_t> mk_pos;
    lazy_buf<uint8_t> mk_red;       /* ... and one flag per ring and scan behind the cells (k_marker_ring_literal) */
    lazy_buf<float> mk_out;         /* single-scan entry point: 361 x 4 floats + 1 count */
    lazy_buf<int32_t> mk_ghost;     /* urf_marker_strips_batch: the incoming ghost count (the call's last scan overwrites the caller's word) */
    uint32_t* compact_cnt = nullptr;   /* [max_batch][max_tiles][4] */
    /* the published clouds of a batch (urf_clouds_batch_*): per (scan, tile) counts and bases, and the ordered lists of the
     * reference order: 3 x scans x stride entries + 3 counts per scan */
    lazy_buf<urf_u32x4> cl_tiles;   /* 2 x [max_batch][max_tiles] */
    lazy_buf<uint32_t> cl_lists;
    /* dense sweeps put back into firing slots (urf_k_dense.hpp), grown by the first dense call: every dense point's position inside its
     * padded scan and the padded batch's labels ([max_batch][max_points] each; the padded x / y / z are the SoA staging), the per-tile
     * and per-scan words (2 x [max_batch][max_tiles] + [max_batch] + 1), the slot map's device copy */
    lazy_buf<uint32_t> dn_pos;
    lazy_buf<uint8_t> dn_labels;
    lazy_buf<uint32_t> dn_words;
    lazy_buf<uint8_t> dn_map;
    /* urf_classify_batch_*_dense_elev: the ids derived from the points' elevation ([max_batch][max_points] bytes, indexed like the
     * caller's arrays) and the device copy of dense_elev, both grown by the first such call */
    lazy_buf<uint8_t> dn_ids;
    lazy_buf<urf_dense_elev_table> dn_elev;
    urf_dense_elev_table dense_elev;   /* urf_set_dense_elevations, for dense_elev_n slots (0: none) */
    uint32_t dense_elev_n = 0;
    bool dense_elev_dirty = true;      /* ... not yet in dn_elev */
    struct { urf_dense_args d; urf_dense_ids_args e; uint32_t kind = URF_LAST_NONE; } dn_ids_call;   /* the last id launch (urf_test_dense_ids_ms) */
    /* urf_set_dense_outputs: the inverse of dn_pos ([max_batch][max_points], k_dense_inverse), grown by the first read-out that needs it
     * and built once per dense call: dn_calls counts those (a rerun of the padded batch writes `last` and leaves dn_pos as it is), dn_inv_of
     * is the one dn_inv holds (0: none) */
    lazy_buf<uint32_t> dn_inv;
    uint64_t dn_calls = 0, dn_inv_of = 0;
    bool dense_outputs = false;
    uint8_t dense_map[256];         /* urf_set_dense_slots (urf_create: the identity); 0xff: no such id */
    bool dense_map_dirty = true;    /* ... not yet in dn_map */
    float* d_newY = nullptr;
    urf_beam* d_beams = nullptr;
    uint32_t beams_cap = 0;
    int capture = 0;                /* urf_enable_stage_capture */
    bool timing = false;
    std::vector<std::vector<hipEvent_t>> timing_events;   /* sets of URF_NUM_KERNELS+1 events, created once and reused */
    size_t timing_used = 0;         /* sets recorded since the last urf_kernel_timing() */
    uint32_t* offsets_copy = nullptr;   /* [max_batch + 1] the ragged offsets of the last call (context-owned) */
    /* k_front_finish's first part runs on a stream of its own next to the star-shaped search (side_fork): all three or none */
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    urf_last_call last;
    urf_planned planned;            /* run_pipeline: the call it planned last (its callers keep it with the call's arguments) */
    /* urf_front_explain: k_front_explain's per-scan records ([scans][URF_FX_WORDS]), grown by its first call */
    lazy_buf<uint32_t> fx_rec;
    /* urf_set_front_auto's learning pass, allocated by the first call that turns the switch on: k_front_explain's records for a batch
     * call (rows 0 .. max_batch - 1) and for the sweep of each slot (row max_batch + slot), k_front_digest's accumulators and its
     * host-mapped digests ([1 + URF_ASYNC_SLOTS][URF_DG_WORDS] each: a batch call's first, then the slots') */
    struct {
        lazy_buf<uint32_t> rec, acc;
        mapped_buf dig;
    } au;
    std::string last_error;
    /* host-side cost of the callback path, phase by phase (only the build with the test hooks fills them:
     * URF_HOST_TIMES=1, printed by its benchmark loop; the context's layout is the same in both builds) */
    double ht[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    bool ht_on = false;
};

#define URF_HIP(ctx, call)                                                              \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return e_ == hipErrorOutOfMemory ? URF_ERR_OOM : URF_ERR_HIP;               \
        }                                                                               \
    } while (0)

/* a slot's captured sequences: released one by one (seq_drop) or all of them (slot_forget); never while the slot's sweep is in flight */
static void seq_drop(urf_ctx::slot_t::seq_t& q)
{
    if (q.exec)
        (void)hipGraphExecDestroy(q.exec);
    if (q.graph)
        (void)hipGraphDestroy(q.graph);
    q.exec = nullptr;
    q.graph = nullptr;
    q.key[0] = 0;
}
static void slot_forget(urf_ctx::slot_t& sl)
{
    for (auto& q : sl.seqs)
        seq_drop(q);
}

template <class T>
static int dev_alloc(urf_ctx* c, T** p, size_t count)
{
    void* v = nullptr;
    URF_HIP(c, hipMalloc(&v, (count ? count : 1) * sizeof(T)));
    c->allocs.push_back(v);
    *p = (T*)v;
    return URF_OK;
}

/* b holds at least `count` elements afterwards.  To grow, it waits for `st` first when one is given (work in flight there may still
 * read the old memory) and frees the old memory; a failed allocation leaves it empty. */
template <class T, bool Host>
static int grow(urf_ctx* c, lazy_buf<T, Host>& b, size_t count, hipStream_t st = nullptr)
{
    if (count <= b.cap)
        return URF_OK;
    if (st)
        URF_HIP(c, hipStreamSynchronize(st));
    b.release();
    void* v = nullptr;
    URF_HIP(c, Host ? hipHostMalloc(&v, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&v, count * sizeof(T)));
    b.p = (T*)v;
    b.cap = count;
    return URF_OK;
}

/* f(group, field, rows, elements per row) for every scratch array of `k` (URF_SCRATCH_*) */
template <class F>
static void scratch_walk(const urf_ctx* c, urf_kargs& k, F&& f)
{
    const size_t sstride = c->sstride, max_tiles = c->max_tiles, max_points = c->max_points, front_cand_cap = k.front_cand_cap;
#define URF_X_SCANS(field, n) f(URF_SCR_ALWAYS, k.field, (size_t)c->max_batch, (size_t)(n));
#define URF_X_SLOTS(field, n) f(URF_SCR_ALWAYS, k.field, (size_t)URF_ASYNC_SLOTS, (size_t)(n));
#define URF_X_CAPTURE(field, n) f(URF_SCR_CAPTURE, k.field, (size_t)c->max_batch, (size_t)(n));
#define URF_X_ROW_MAJOR(field, n) f(URF_SCR_ROW_MAJOR, k.field, (size_t)c->max_batch, (size_t)(n));
#define URF_X_LASERS128(field, n) f(URF_SCR_LASERS128, k.field, (size_t)c->max_batch, (size_t)(n));
#define URF_X_MULTI_SECTOR(field, n) f(URF_SCR_MULTI_SECTOR, k.field, (size_t)c->max_batch, (size_t)(n));
    URF_SCRATCH_SCANS(URF_X_SCANS)
    URF_SCRATCH_SLOTS(URF_X_SLOTS)
    URF_SCRATCH_CAPTURE(URF_X_CAPTURE)
    URF_SCRATCH_ROW_MAJOR(URF_X_ROW_MAJOR)
    URF_SCRATCH_LASERS128(URF_X_LASERS128)
    URF_SCRATCH_MULTI_SECTOR(URF_X_MULTI_SECTOR)
#undef URF_X_SCANS
#undef URF_X_SLOTS
#undef URF_X_CAPTURE
#undef URF_X_ROW_MAJOR
#undef URF_X_LASERS128
#undef URF_X_MULTI_SECTOR
}

/* Allocates the arrays of `group` that are missing (URF_OK: all of them are there). */
static int scratch_alloc(urf_ctx* c, urf_scratch_group group)
{
    int rc = URF_OK;
    scratch_walk(c, c->k, [&](urf_scratch_group g, auto*& p, size_t rows, size_t n) {
        if (g == group && !p && rc == URF_OK)
            rc = dev_alloc(c, &p, rows * n);
    });
    return rc;
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
    std::memset(&c->last.a, 0, sizeof(c->last.a));
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
        slot_forget(sl);
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
    c->pol.front_outputs = on != 0;   /* (the read-outs' scratch grows with their first use: front_out_prepare) */
    return URF_OK;
}

/* ---- urf_set_sweep_outputs (include/urf.h) ---------------------------------------------------- */
/* A slot's result buffer, in 32-bit words: the marker points (URF_DEG_CELLS x 4 floats), their count, the three list counts -- one small
 * copy --, then the road, curb and ring-10 lists at a stride of the sweep's n_points (one copy of 3 x n_points words, sized at capture). */
#define URF_SWEEP_HDR_MCOUNT (URF_DEG_CELLS * 4u)
#define URF_SWEEP_HDR_LCOUNTS (URF_SWEEP_HDR_MCOUNT + 1u)
#define URF_SWEEP_HDR (URF_SWEEP_HDR_LCOUNTS + 3u)
#define URF_DBG_SWEEP_OLD_KERNELS 32u   /* test hook (urf_set_debug_flags): with both bits set the sequence launches the kernels of the two
                                           products one by one instead of k_sweep_rings / k_sweep_lists (A/B, tools/sweep_outputs_bench.py) */
static uint32_t sweep_rows(const urf_ctx* c) { return c->max_batch < URF_ASYNC_SLOTS ? c->max_batch : URF_ASYNC_SLOTS; }

/* Everything the sequences will need, before any of them is captured: nothing may be allocated inside a stream capture.  The buffers are
 * of fixed size (rows, sstride, max_points): a second call finds them there. */
static int sweep_outputs_alloc(urf_ctx* c, bool direct)
{
    const size_t rows = sweep_rows(c), cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS, ss = c->sstride;
    urf_ctx::sweep_scratch_t& w = c->sweep;
    int rc;
    if ((rc = grow(c, w.mk_d, rows * cells)) != URF_OK || (rc = grow(c, w.mk_pos, rows * cells)) != URF_OK ||
        (rc = grow(c, w.mk_red, rows * (cells + URF_MAX_CHANNELS))) != URF_OK || (rc = grow(c, w.ord_keys, rows * ss)) != URF_OK ||
        (rc = grow(c, w.ord_pos, rows * ss)) != URF_OK || (rc = grow(c, w.ord_cls, rows * URF_MAX_CHANNELS * 2)) != URF_OK ||
        (rc = grow(c, w.fo_az, rows * ss)) != URF_OK || (rc = grow(c, w.fo_ent, rows * ss)) != URF_OK || (rc = grow(c, w.fo_d, rows * ss)) != URF_OK)
        return rc;
    if (direct) {   /* (urf_set_sweep_results_direct: the kernels' own stores, no device-side result buffer) */
        const size_t words = URF_SWEEP_HDR + 2 * (size_t)c->max_points;
        for (auto& sl : c->slots) {
            mapped_buf& m = sl.m_out;
            if (m.cap >= words)
                continue;
            m.release();
            void *hp = nullptr, *dp_ = nullptr;
            URF_HIP(c, hipHostMalloc(&hp, words * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
            m.p = (uint32_t*)hp;
            URF_HIP(c, hipHostGetDevicePointer(&dp_, hp, 0));
            m.dev = (uint32_t*)dp_;
            m.cap = words;
            std::memset(m.p, 0, URF_SWEEP_HDR * sizeof(uint32_t));   /* (a sweep with one bit set leaves the other product's words alone) */
        }
        return URF_OK;
    }
    const size_t words = URF_SWEEP_HDR + 3 * (size_t)c->max_points;
    for (auto& sl : c->slots) {
        const bool fresh = sl.d_out.cap < words;
        if ((rc = grow(c, sl.d_out, words)) != URF_OK || (rc = grow(c, sl.h_out, words)) != URF_OK)
            return rc;
        if (fresh) {   /* (a sweep with one bit set copies the whole header) */
            URF_HIP(c, hipMemset(sl.d_out.p, 0, URF_SWEEP_HDR * sizeof(uint32_t)));
            std::memset(sl.h_out.p, 0, URF_SWEEP_HDR * sizeof(uint32_t));
        }
    }
    return URF_OK;
}

extern "C" int urf_set_sweep_outputs(urf_ctx* c, uint32_t bits)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    if (bits & ~(URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER)) {
        c->last_error = "urf_set_sweep_outputs: bits other than URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER";
        return URF_ERR_INVALID_ARG;
    }
    for (const auto& sl : c->slots)
        if (sl.pending) {
            c->last_error = "urf_set_sweep_outputs: a sweep is in flight (urf_classify_pc2_wait it first)";
            return URF_ERR_BUSY;
        }
    if (bits) {
        URF_HIP(c, hipSetDevice(c->device));
        const int rc = sweep_outputs_alloc(c, c->pol.sweep_direct);
        if (rc != URF_OK)
            return rc;   /* (the switch stays as it was) */
    }
    c->pol.set(c->pol.sweep_outputs, bits);   /* (every slot captures its sequence again) */
    return URF_OK;
}

/* ---- urf_set_sweep_results_direct (include/urf.h) ---------------------------------------------- */
/* Whichever of the two setters comes second allocates the result buffers of the layout that is then in force (sweep_outputs_alloc), outside
 * any capture; with no bit of urf_set_sweep_outputs set this one allocates nothing. */
extern "C" int urf_set_sweep_results_direct(urf_ctx* c, int on)
{
    if (!c || (on != 0 && on != 1))
        return URF_ERR_INVALID_ARG;
    for (const auto& sl : c->slots)
        if (sl.pending) {
            c->last_error = "urf_set_sweep_results_direct: a sweep is in flight (urf_classify_pc2_wait it first)";
            return URF_ERR_BUSY;
        }
    if (c->pol.sweep_outputs && (on != 0) != c->pol.sweep_direct) {
        URF_HIP(c, hipSetDevice(c->device));
        const int rc = sweep_outputs_alloc(c, on != 0);
        if (rc != URF_OK)
            return rc;   /* (the switch stays as it was) */
    }
    c->pol.set(c->pol.sweep_direct, on != 0);   /* (every slot captures its sequence again) */
    return URF_OK;
}

/* ---- urf_set_sweep_quantum, urf_callback_path_captures (include/urf.h) ------------------------- */
extern "C" int urf_set_sweep_quantum(urf_ctx* c, uint32_t points)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    if (points % URF_TILE != 0u || points > c->max_points) {
        c->last_error = "urf_set_sweep_quantum: not a multiple of URF_TILE (2048) points, or more than the context's max_points";
        return URF_ERR_INVALID_ARG;
    }
    for (const auto& sl : c->slots)
        if (sl.pending) {
            c->last_error = "urf_set_sweep_quantum: a sweep is in flight (urf_classify_pc2_wait it first)";
            return URF_ERR_BUSY;
        }
    if (points) {   /* the slots' length words, before any sequence is captured */
        URF_HIP(c, hipSetDevice(c->device));
        for (auto& sl : c->slots) {
            int rc;
            if ((rc = grow(c, sl.h_n, 1)) != URF_OK || (rc = grow(c, sl.d_n, 1)) != URF_OK)
                return rc;   /* (the switch stays as it was) */
        }
    }
    c->pol.set(c->pol.sweep_quantum, points);   /* (a change: every slot forgets its sequences with its next sweep) */
    return URF_OK;
}

extern "C" int urf_callback_path_captures(const urf_ctx* c, uint32_t* n_captured, uint32_t* n_resident)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    if (n_captured)
        *n_captured = c->n_captured;
    if (n_resident) {   /* (a sequence of an earlier epoch is no sweep's any more: its slot's next submission releases it) */
        *n_resident = 0;
        for (const auto& sl : c->slots)
            for (const auto& q : sl.seqs)
                *n_resident += (q.exec && q.key[0] == c->pol.epoch) ? 1u : 0u;
    }
    return URF_OK;
}

extern "C" int urf_front_scans(urf_ctx* c, uint32_t* n_fused)
{
    if (!c || !n_fused)
        return URF_ERR_INVALID_ARG;
    *n_fused = 0;
    if (!c->last.a.front)   /* (or no call yet) */
        return URF_OK;
    URF_HIP(c, hipSetDevice(c->device));
    URF_HIP(c, hipStreamSynchronize(c->stream));   /* (a sweep of the callback path has been waited for: its row is at rest) */
    std::vector<uint32_t> ok(c->last.scans);
    URF_HIP(c, hipMemcpy(ok.data(), c->last.a.front_ok, ok.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
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

/* The context's scratch at row `row` (URF_SCRATCH_*): slot i of the callback path (URF_MAX_IN_FLIGHT slots) runs on row
 * i % min(max_batch, URF_MAX_IN_FLIGHT) and on that row's own stream, so that the sweeps in flight overlap.  Row 0 = the
 * context's own arguments; a lazy group that is not there stays NULL. */
static urf_kargs kargs_row(const urf_ctx* c, uint32_t row)
{
    urf_kargs k = c->k;
    if (row)
        scratch_walk(c, k, [&](urf_scratch_group, auto*& p, size_t, size_t n) {
            if (p)
                p += row * n;
        });
    return k;
}

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
static int auto_pass(urf_ctx* c, const urf_kargs& a, const urf_dev_params& dp, const urf_planned& planned, hipStream_t st, uint32_t which,
                     uint32_t rec_row, uint32_t sweep_n)
{
    urf_policy& p = c->pol;
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
    hipLaunchKernelGGL(k_front_explain, dim3(a.tiles, n), dim3(64), 0, st, a, dp, rows ? 1u : 0u, rec);
    hipLaunchKernelGGL(k_front_digest, dim3((n + 255u) / 256u), dim3(256), 0, st, a, fx_call_of(a, dp, planned, rows, sweep_n), rec, acc,
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

/* The launch sequence of one call as the policy plans it; the arguments and parameters it ran with go to a_out / dp_out, last of all and
 * only for a call that succeeded and was not empty (call.dp may point at dp_out, the call's values may come from a_out: the two reruns) */
static int run_pipeline(urf_ctx* c, const urf_call& call, urf_kargs& a_out, urf_dev_params& dp_out)
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
    urf_kargs a = kargs_row(c, call.row);
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
    const urf_dev_params dp = call.dp ? *call.dp : c->dp;
    const unsigned C = (unsigned)dp.p.channels, K = (unsigned)dp.p.sectors;
    const bool star = dp.p.star_shaped_method != 0;
    const dim3 g_tiles(a.tiles, n_scans), g_scan(n_scans);
    c->pol.plan(a, dp, slot, call.general_only);
    c->planned = urf_planned{ c->pol.why(a, dp, slot, call.general_only), c->pol.ms_ok(dp) };   /* (host words for urf_front_explain: decides nothing) */
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
        const int rc = auto_pass(c, a, dp, c->planned, st, 0u, call.row, 0u);
        if (rc != URF_OK)
            return rc;
    }
    a_out = a;
    dp_out = dp;
    return URF_OK;
}

static void publish_last(urf_ctx* c, int kind, uint32_t scans, const urf_kargs& a, const urf_dev_params& dp, const urf_planned& planned, uint32_t row = 0,
                         uint64_t gen = 0)
{
    c->last = urf_last_call{ kind, scans, a, dp, row, gen, planned };
    c->last_seq++;
}

/* a call of the public batch entry points: published after a successful call that was not empty (an empty one leaves the last call as it was) */
static int classify_batch(urf_ctx* c, int kind, const urf_call& call)
{
    urf_kargs a;
    urf_dev_params dp;
    const int rc = run_pipeline(c, call, a, dp);
    if (rc == URF_OK && call.n_scans)
        publish_last(c, kind, call.n_scans, a, dp, c->planned);
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

/* ---- the callback path: one sweep, host buffers ------------------------------- */
/* Slot i of the callback path works on scratch row i % rows, rows = min(max_batch, URF_ASYNC_SLOTS), and on
 * that row's compute stream (row 0: the context's stream): with a context created for several scans the
 * kernels of as many sweeps overlap on the device (a single sweep's kernels are a few dozen workgroups
 * each).  With max_batch == 1 all slots share row 0 and the context's stream: only the copies overlap. */
static uint32_t slot_row(const urf_ctx* c, const urf_ctx::slot_t& sl)
{
    const uint32_t rows = c->max_batch < URF_ASYNC_SLOTS ? c->max_batch : URF_ASYNC_SLOTS;
    return (uint32_t)(&sl - c->slots) % rows;
}
static hipStream_t slot_stream(urf_ctx* c, const urf_ctx::slot_t& sl)
{
    const uint32_t row = slot_row(c, sl);
    return row ? c->row_stream[row] : c->stream;
}

static int slot_prepare(urf_ctx* c, urf_ctx::slot_t& sl, size_t bytes)
{
    if (!c->streams_made) {
        for (uint32_t r = 1; r < URF_ASYNC_SLOTS && r < c->max_batch; r++)
            URF_HIP(c, hipStreamCreateWithFlags(&c->row_stream[r], hipStreamNonBlocking));
        c->streams_made = true;
    }
    if (!sl.ev_done)
        URF_HIP(c, hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
    int rc;
    if ((rc = grow(c, sl.h_labels, c->max_points)) != URF_OK || (rc = grow(c, sl.h_info, 1)) != URF_OK ||
        (rc = grow(c, sl.d_labels, c->max_points)) != URF_OK)
        return rc;
    if (bytes > sl.h_in.cap || bytes > sl.d_raw.cap) {   /* grows to the largest message seen (a new buffer invalidates the captured sequences) */
        for (auto& q : sl.seqs)
            q.key[0] = 0;
        const hipStream_t st = slot_stream(c, sl);   /* the slot's last sweep may still read d_raw */
        if ((rc = grow(c, sl.h_in, bytes, st)) != URF_OK || (rc = grow(c, sl.d_raw, bytes, st)) != URF_OK)
            return rc;
    }
    return URF_OK;
}

#ifdef URF_ENABLE_TEST_HOOKS
static inline double ht_now()
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
#define HT_START double ht0 = c->ht_on ? ht_now() : 0.0
#define HT(k, t0) do { if (c->ht_on) { const double ht_t = ht_now(); c->ht[k] += ht_t - (t0); (t0) = ht_t; } } while (0)
#else
#define HT_START
#define HT(k, t0)
#endif

/* A message that has to be staged anyway is staged as three planes x[n4] y[n4] z[n4], n4 = n rounded up to 4: 12 of
 * its (typically) 32 bytes per point cross PCIe (84 -> 35 us for a 64 x 2048 sweep), and the device needs no
 * records -> SoA kernel.  Records whose x, y, z lie side by side with a fourth word behind them inside the record
 * (pcl::PointXYZI and every PointCloud2 layout of the lidar drivers) go four at a time through a 4 x 4 transpose and
 * leave with non-temporal stores (the planes are 16-byte aligned; on the test box's EPYC 9575F: memcpy of the 4 MiB
 * message 108 us, the transpose with ordinary stores 105, with streaming stores 67). */
static void pc2_to_planes(const uint8_t* data, uint32_t i0, uint32_t n, uint32_t step, uint32_t ox, uint32_t oy, uint32_t oz, float* X,
                          float* Y, float* Z)   /* points [i0, n); i0 a multiple of 4 */
{
    uint32_t i = i0;
#if defined(__SSE2__)
    if (oy == ox + 4 && oz == ox + 8 && (uint64_t)ox + 16 <= step) {
        const uint8_t* p = data + (size_t)i0 * step + ox;
        if ((((uintptr_t)(X + i0) | (uintptr_t)(Y + i0) | (uintptr_t)(Z + i0)) & 15u) == 0) {   /* (the pinned planes: always) */
            for (; i + 4 <= n; i += 4, p += 4 * (size_t)step) {
                __m128 r0 = _mm_loadu_ps((const float*)p), r1 = _mm_loadu_ps((const float*)(p + step));
                __m128 r2 = _mm_loadu_ps((const float*)(p + 2 * (size_t)step)), r3 = _mm_loadu_ps((const float*)(p + 3 * (size_t)step));
                _MM_TRANSPOSE4_PS(r0, r1, r2, r3);
                _mm_stream_ps(X + i, r0);
                _mm_stream_ps(Y + i, r1);
                _mm_stream_ps(Z + i, r2);
            }
            _mm_sfence();   /* before the DMA engine is told to read them */
        } else {
            for (; i + 4 <= n; i += 4, p += 4 * (size_t)step) {
                __m128 r0 = _mm_loadu_ps((const float*)p), r1 = _mm_loadu_ps((const float*)(p + step));
                __m128 r2 = _mm_loadu_ps((const float*)(p + 2 * (size_t)step)), r3 = _mm_loadu_ps((const float*)(p + 3 * (size_t)step));
                _MM_TRANSPOSE4_PS(r0, r1, r2, r3);
                _mm_storeu_ps(X + i, r0);
                _mm_storeu_ps(Y + i, r1);
                _mm_storeu_ps(Z + i, r2);
            }
        }
    }
#endif
    for (; i < n; i++) {
        const uint8_t* p = data + (size_t)i * step;
        std::memcpy(X + i, p + ox, 4);
        std::memcpy(Y + i, p + oy, 4);
        std::memcpy(Z + i, p + oz, 4);
    }
}

/* the gather by itself (host only, no context): what urf_classify_pc2_async does with a message it stages */
extern "C" int urf_pc2_to_planes(const uint8_t* data, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                                 uint32_t off_z, float* x, float* y, float* z)
{
    if (!data || !x || !y || !z || !pc2_layout_ok(point_step, off_x, off_y, off_z))
        return URF_ERR_INVALID_ARG;
    pc2_to_planes(data, 0, n_points, point_step, off_x, off_y, off_z, x, y, z);
    return URF_OK;
}

/* urf_set_sweep_outputs: the read-outs of the sweep run_pipeline has just launched on `st`, behind it on the same stream -- one linear
 * chain, separate launches as the only synchronisation -- with the sweep's own arguments and parameters (sl.cap_a: its scratch row, scan
 * 0), the row's read-out scratch and the slot's result buffers; then the copies to the slot's pinned buffer.  The kernels are
 * launch_markers' / launch_ordered's: a fused sequence (cap_a.front) holds the pre-pass and the *_front siblings as well and the scan
 * decides on the device which of each pair works; a sweep the short sequence voided leaves empty results (every kernel returns for a
 * status that is not URF_OK) and gets the right ones from its rerun.  With both bits set the per-ring work of the two products is one
 * launch (k_sweep_rings), lists and marker points another (k_sweep_lists).  c->fo_prep and want_ring_sorted are none of its business. */
static int sweep_outputs_launch(urf_ctx* c, urf_ctx::slot_t& sl, uint32_t row, hipStream_t st, uint32_t n_points)
{
    const uint32_t bits = c->pol.sweep_outputs;
    if (!bits)
        return URF_OK;
    const urf_kargs& a = sl.cap_a;
    const urf_dev_params& dp = sl.cap_dp;
    const bool mark = (bits & URF_SWEEP_OUT_MARKER_POINTS) != 0, order = (bits & URF_SWEEP_OUT_ORDER) != 0, fused = a.front != 0;
    const bool merged = mark && order && !(c->debug_flags & URF_DBG_SWEEP_OLD_KERNELS);
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS, ss = c->sstride;
    urf_ctx::sweep_scratch_t& w = c->sweep;
    float* const mk_d = w.mk_d.p + row * cells;
    uint32_t* const mk_pos = w.mk_pos.p + row * cells;
    uint8_t* const mk_red = w.mk_red.p + row * (cells + URF_MAX_CHANNELS);
    uint8_t* const mk_lit = mk_red + cells;
    unsigned long long* const ord_keys = w.ord_keys.p + row * ss;
    uint32_t* const ord_pos = w.ord_pos.p + row * ss;
    uint32_t* const ord_cls = w.ord_cls.p + (size_t)row * URF_MAX_CHANNELS * 2;
    uint32_t* const fo_az = w.fo_az.p + row * ss;
    uint32_t* const fo_ent = w.fo_ent.p + row * ss;
    float* const fo_d = w.fo_d.p + row * ss;
    /* urf_set_sweep_results_direct: the slot's mapped pinned buffer as the device sees it -- the last kernels of the chain store header
     * results and lists there themselves, the lists back to back (k_sweep_lists_direct / k_ordered_lists_direct), and nothing is copied */
    const bool direct = c->pol.sweep_direct;
    uint32_t* const out = direct ? sl.m_out.dev : sl.d_out.p;
    float* const d_pts = (float*)out;
    uint32_t* const d_mcount = out + URF_SWEEP_HDR_MCOUNT;
    uint32_t* const d_lcounts = out + URF_SWEEP_HDR_LCOUNTS;
    uint32_t* const d_road = out + URF_SWEEP_HDR;
    uint32_t* const d_curb = d_road + n_points;
    uint32_t* const d_r10 = d_curb + n_points;
    const dim3 g_ring((unsigned)dp.p.channels, 1), b256(256);
    const size_t map_lds = (2 * (size_t)a.tiles + 1) * sizeof(unsigned);
    if (fused)
        hipLaunchKernelGGL(k_front_out_prep, dim3(a.tiles, 1), b256, 0, st, a, dp, 0u, fo_az, fo_ent, fo_d);
    if (merged) {
        hipLaunchKernelGGL(k_sweep_rings, g_ring, b256, map_lds, st, a, dp, urf_ring_outs{ ord_keys, ord_pos, ord_cls, mk_d, mk_pos, mk_red, mk_lit });
    } else {
        if (order)
            hipLaunchKernelGGL(k_ring_order, g_ring, b256, map_lds, st, a, dp, 0u, ord_keys, ord_pos, ord_cls);
        if (mark)
            hipLaunchKernelGGL(k_marker_ring, g_ring, b256, map_lds, st, a, dp, 0u, mk_d, mk_pos, mk_red, mk_lit);
    }
    if (fused && order)
        hipLaunchKernelGGL(k_ring_order_front, g_ring, b256, 0, st, a, dp, 0u, fo_az, fo_ent, ord_pos, ord_cls);
    if (fused && mark)
        hipLaunchKernelGGL(k_marker_ring_front, g_ring, b256, 0, st, a, dp, 0u, fo_az, fo_ent, fo_d, mk_d, mk_pos, mk_red, mk_lit);
    if (mark) {   /* rings in which the ORDER of equal azimuths decides a marker point (normally none: every workgroup returns at once) */
        hipLaunchKernelGGL(k_marker_ring_literal, g_ring, b256, 0, st, a, dp, 0u, mk_lit, mk_d, mk_pos, mk_red);
        if (fused)
            hipLaunchKernelGGL(k_marker_ring_literal_front, g_ring, b256, 0, st, a, dp, 0u, mk_lit, fo_az, fo_ent, fo_d, mk_d, mk_pos, mk_red);
    }
    if (merged) {
        if (direct)
            hipLaunchKernelGGL(k_sweep_lists_direct, dim3((unsigned)dp.p.channels + 1u, 1), dim3(384), 0, st, a, dp,
                               urf_sweep_lists_args{ ord_pos, ord_cls, d_road, nullptr, nullptr, d_lcounts, 0u, mk_d, mk_pos, mk_red, d_pts, d_mcount });
        else
            hipLaunchKernelGGL(k_sweep_lists, dim3((unsigned)dp.p.channels + 1u, 1), dim3(384), 0, st, a, dp,
                               urf_sweep_lists_args{ ord_pos, ord_cls, d_road, d_curb, d_r10, d_lcounts, n_points, mk_d, mk_pos, mk_red, d_pts, d_mcount });
    } else {
        if (order && direct)
            hipLaunchKernelGGL(k_ordered_lists_direct, g_ring, b256, 0, st, a, dp, ord_pos, ord_cls, d_road, d_lcounts);
        else if (order)
            hipLaunchKernelGGL(k_ordered_lists, g_ring, b256, 0, st, a, dp, 0u, ord_pos, ord_cls, d_road, d_curb, d_r10, n_points, d_lcounts);
        if (mark) {
            hipLaunchKernelGGL(k_marker_bins, dim3(1), dim3(384), 0, st, a, dp, 0u, mk_d, mk_pos, mk_red, d_pts, d_mcount);
            if (fused)
                hipLaunchKernelGGL(k_marker_bins_front, dim3(1), dim3(384), 0, st, a, dp, 0u, mk_d, mk_pos, mk_red, d_pts, d_mcount);
        }
    }
    URF_HIP(c, hipGetLastError());
    if (direct)
        return URF_OK;   /* (the results are where the host reads them once the slot's event has completed) */
    URF_HIP(c, hipMemcpyAsync(sl.h_out.p, out, URF_SWEEP_HDR * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (order)
        URF_HIP(c, hipMemcpyAsync(sl.h_out.p + URF_SWEEP_HDR, d_road, 3 * (size_t)n_points * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return URF_OK;
}

/* what one sweep of the callback path launches on the compute stream: records -> SoA (unless the message was
 * staged as planes), the pipeline, results to the pinned host buffers */
static int slot_launch(urf_ctx* c, urf_ctx::slot_t& sl, uint32_t n_points, uint32_t point_step, uint32_t off_x,
                       uint32_t off_y, uint32_t off_z, const urf_dev_params* dp_in = nullptr, int capture_in = -1)
{
    const uint32_t row = slot_row(c, sl);
    hipStream_t st = slot_stream(c, sl);
    float *sx, *sy, *sz;
    if (sl.planes) {
        const size_t n4 = ((size_t)n_points + 3) & ~(size_t)3;
        sx = (float*)sl.d_raw.p;
        sy = sx + n4;
        sz = sy + n4;
    } else {
        sx = c->sx.p + (size_t)row * c->max_points;   /* (ensure_soa_staging: the caller) */
        sy = c->sy.p + (size_t)row * c->max_points;
        sz = c->sz.p + (size_t)row * c->max_points;
        if (sl.pad)   /* (urf_set_sweep_quantum: n_points is the padded length, the sweep's own stands in the slot's device word) */
            hipLaunchKernelGGL(k_pc2_to_soa_pad, dim3((n_points + 255) / 256), dim3(256), 0, st, sl.d_raw.p, sl.d_n.p, n_points, point_step,
                               off_x, off_y, off_z, sx, sy, sz);
        else
            hipLaunchKernelGGL(k_pc2_to_soa, dim3((n_points + 255) / 256), dim3(256), 0, st, sl.d_raw.p, (unsigned long long)n_points,
                               point_step, off_x, off_y, off_z, sx, sy, sz);
    }
    const int rc = run_pipeline(c, urf_call{ sx, sy, sz, nullptr, n_points, n_points, 1, sl.d_labels.p, nullptr, row, st, dp_in, capture_in },
                                sl.cap_a, sl.cap_dp);
    if (rc != URF_OK)
        return rc;
    sl.cap_planned = c->planned;
    URF_HIP(c, hipMemcpyAsync(sl.h_labels.p, sl.d_labels.p, n_points, hipMemcpyDeviceToHost, st));
    URF_HIP(c, hipMemcpyAsync(sl.h_info.p, kargs_row(c, row).info, sizeof(urf_scan_info), hipMemcpyDeviceToHost, st));
    return sweep_outputs_launch(c, sl, row, st, n_points);   /* (urf_set_sweep_outputs; off: nothing) */
}

extern "C" int urf_pinned_input(urf_ctx* c, size_t bytes, uint8_t** ptr)
{
    if (!c || !ptr || bytes == 0)
        return URF_ERR_INVALID_ARG;
    urf_ctx::slot_t& sl = c->slots[c->next_ticket % URF_ASYNC_SLOTS];   /* the slot the next submission uses */
    if (sl.pending)
        return URF_ERR_BUSY;
    URF_HIP(c, hipSetDevice(c->device));
    const int rc = slot_prepare(c, sl, bytes);
    if (rc != URF_OK)
        return rc;
    *ptr = sl.h_in.p;
    return URF_OK;
}

extern "C" int urf_classify_pc2_async(urf_ctx* c, const uint8_t* data, uint32_t n_points, uint32_t point_step,
                                      uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t* ticket)
{
    if (!c || !data || !ticket || n_points == 0 || !pc2_layout_ok(point_step, off_x, off_y, off_z))
        return URF_ERR_INVALID_ARG;   /* before any byte of the message is copied */
    if (n_points > c->max_points)
        return URF_ERR_CAPACITY;
    urf_ctx::slot_t& sl = c->slots[c->next_ticket % URF_ASYNC_SLOTS];
    if (sl.pending)
        return URF_ERR_BUSY;          /* every slot in flight: urf_classify_pc2_wait() the oldest one first */
    URF_HIP(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n_points * point_step;
    HT_START;
    /* a message inside the slot's pinned buffer must be the buffer urf_pinned_input() handed out, and
     * fit it: a larger one would make slot_prepare() free the very memory it is about to read */
    if (sl.h_in.p && data >= sl.h_in.p && data < sl.h_in.p + sl.h_in.cap && (data != sl.h_in.p || bytes > sl.h_in.cap))
        return URF_ERR_INVALID_ARG;
    const bool planes = data != sl.h_in.p;   /* (a producer that filled the pinned buffer itself wrote records) */
    /* urf_set_sweep_quantum: the sweep runs as the next multiple of the quantum, (NaN, NaN, NaN) behind its own points -- the reference
     * drops non-finite points before anything else, so labels and summary are those of the unpadded sweep -- and every sweep of that
     * padded length replays one captured sequence.  A padded length beyond max_points: unpadded, under its own key. */
    uint32_t n_run = n_points;
    bool pad = false;
    if (const uint32_t q = c->pol.sweep_quantum) {
        const uint64_t up = ((uint64_t)n_points + q - 1) / q * q;
        if (up <= c->max_points) {
            n_run = (uint32_t)up;
            pad = true;   /* (a multiple of the quantum too: it shares the padded sequence of its length) */
        }
    }
    const size_t n4 = ((size_t)n_run + 3) & ~(size_t)3;
    const size_t plane_bytes = 3 * sizeof(float) * n4;
    size_t want = planes && plane_bytes > bytes ? plane_bytes : bytes;
    if (pad && (want > sl.h_in.cap || want > sl.d_raw.cap)) {
        /* a new buffer forgets the slot's sequences, and the messages of such a stream keep growing by a few points: room for twice the
         * padded length (at most max_points), so that the lengths to come fit the buffer this one gets */
        const size_t room = std::min<size_t>(2 * (size_t)n_run, c->max_points);
        want = std::max(want, ((room + 3) & ~(size_t)3) * std::max<size_t>(point_step, 3 * sizeof(float)));
    }
    int rc = slot_prepare(c, sl, want);
    if (rc == URF_OK && !planes)
        rc = ensure_soa_staging(c);   /* where the device gathers the records' x / y / z */
    if (rc != URF_OK)
        return rc;
    hipStream_t st = slot_stream(c, sl);
    rc = order_row_after_main(c, slot_row(c, sl), st);
    if (rc != URF_OK)
        return rc;
    /* The message goes to the device on the slot's own stream, in front of the sweep's kernels.  (r2 / r3 used a copy
     * stream of its own and an event per sweep for the slot's stream to wait on: 7 870 -> 8 670 sweeps/s with a pinned
     * producer, 6 460 -> 7 540 staged without them.  The four streams still map to three hardware queues -- kernel
     * trace, profiles/r3_callback_trace_after.txt --, but more queues made things worse, see profiles/README.md.)
     * Sweeps of other slots run beside the copy as before. */
    if (planes) {
        /* gathered into the pinned planes (pc2_to_planes) in two halves, so that the first one is on its way while the
         * second one is gathered (one 2-D copy per half: its columns of the three planes; 35 us for the whole, 22 per
         * half).  (urf_pinned_input() lets a producer write its records into the pinned buffer directly: no staging.) */
        float* X = (float*)sl.h_in.p;
        const size_t real4 = ((size_t)n_points + 3) & ~(size_t)3;   /* (the halves are halves of the sweep's own points; no pad: n4) */
        const uint32_t mid = n_points >= 32768 ? (uint32_t)((real4 / 2) & ~(size_t)3) : 0u;
        const uint32_t cut[3] = { 0u, mid, n_points };
        for (int h = mid ? 0 : 1; h < 2; h++) {
            pc2_to_planes(data, cut[h], cut[h + 1], point_step, off_x, off_y, off_z, X, X + n4, X + 2 * n4);
            if (h == 1 && n_run != n_points) {   /* the pad: the planes' tails, which the second copy's columns [mid, n_run) carry */
                const float nan = std::numeric_limits<float>::quiet_NaN();
                for (float* P : { X, X + n4, X + 2 * n4 })
                    std::fill(P + n_points, P + n_run, nan);
            }
            const size_t w = (h == 1 ? n4 - cut[1] : cut[1]) * sizeof(float), o = cut[h] * sizeof(float);
            URF_HIP(c, hipMemcpy2DAsync(sl.d_raw.p + o, n4 * sizeof(float), sl.h_in.p + o, n4 * sizeof(float), w, 3, hipMemcpyHostToDevice, st));
        }
    } else {
        URF_HIP(c, hipMemcpyAsync(sl.d_raw.p, sl.h_in.p, bytes, hipMemcpyHostToDevice, st));
        if (pad) {   /* the sweep's own length for k_pc2_to_soa_pad: a word of the slot, copied in front of every launch of the sequence */
            *sl.h_n.p = n_points;
            URF_HIP(c, hipMemcpyAsync(sl.d_n.p, sl.h_n.p, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
    }
    if (planes != sl.planes)
        for (auto& q : sl.seqs)
            q.key[0] = 0;   /* the captured sequences read the other format */
    sl.planes = planes;
    sl.n_run = n_run;
    sl.pad = pad;
    HT(0, ht0);   /* staging + H2D enqueue */
    /* what earlier calls reported, for this sweep and the replayed sequences (outside the stream capture: fold may synchronise) */
    rc = c->pol.fold(c, st);
    if (rc != URF_OK)
        return rc;
    c->pol.probation_sweep();
    if (c->pol.auto_on)   /* urf_set_front_auto: the sweep's advice, applied before its sequence is chosen (a change bumps the epoch) */
        auto_at_call(c, std::max<uint32_t>((n_run + URF_TILE - 1) / URF_TILE, 1u), 1u, (uint32_t)c->capture, true);
    /* the launch sequence of a sweep of this shape is captured once and replayed (one graph launch
     * instead of a dozen kernel launches per callback); anything it depends on bumps the epoch */
    const uint64_t key[3] = { c->pol.epoch,((uint64_t)n_run << 32) | point_step,
                              ((uint64_t)off_x << 42) ^ ((uint64_t)off_y << 21) ^ off_z };
    const bool use_graph = !c->timing && !(c->debug_flags & 8u);
    HT(1, ht0);   /* event record, ordering, stream wait */
    if (use_graph) {
        /* The slot's sequence for this key.  One per slot; with urf_set_sweep_quantum up to URF_SWEEP_SEQS, the least recently used
         * one making room for a new length.  Sequences of an earlier epoch go, all of them, whatever the key. */
        const unsigned n_seqs = c->pol.sweep_quantum ? URF_SWEEP_SEQS : 1u;
        urf_ctx::slot_t::seq_t *seq = nullptr, *room = nullptr;
        for (auto& q : sl.seqs) {
            if (q.exec && q.key[0] != key[0])
                seq_drop(q);
            if (q.exec && q.key[1] == key[1] && q.key[2] == key[2])
                seq = &q;
        }
        if (!seq) {
            for (unsigned i = 0; i < n_seqs; i++) {
                urf_ctx::slot_t::seq_t& q = sl.seqs[i];
                if (!q.exec) {
                    room = &q;
                    break;
                }
                if (!room || q.used < room->used)
                    room = &q;
            }
            seq_drop(*room);
            URF_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
            rc = slot_launch(c, sl, n_run, point_step, off_x, off_y, off_z);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(st, &g);
            if (rc != URF_OK || e != hipSuccess) {
                if (g)
                    (void)hipGraphDestroy(g);
                if (rc == URF_OK)
                    URF_HIP(c, e);
                return rc;
            }
            room->graph = g;
            URF_HIP(c, hipGraphInstantiate(&room->exec, room->graph, nullptr, nullptr, 0));
            room->key[0] = key[0];
            room->key[1] = key[1];
            room->key[2] = key[2];
            room->cap_a = sl.cap_a;
            room->cap_dp = sl.cap_dp;
            room->cap_planned = sl.cap_planned;
            c->n_captured++;
            seq = room;
        } else {   /* (what the sweep in this slot ran with: the readers' record, the rerun's parameters) */
            sl.cap_a = seq->cap_a;
            sl.cap_dp = seq->cap_dp;
            sl.cap_planned = seq->cap_planned;
        }
        seq->used = ++c->seq_clock;
        URF_HIP(c, hipGraphLaunch(seq->exec, st));
    } else {
        rc = slot_launch(c, sl, n_run, point_step, off_x, off_y, off_z);
        if (rc != URF_OK)
            return rc;
    }
    HT(2, ht0);   /* graph launch (or the launches themselves) */
    /* urf_set_front_auto's learning pass: no part of the captured sequence, on the sweep's stream behind it and in front of ev_done --
     * the event urf_classify_pc2_wait waits for, the context's stream waits for before it touches a row (order_after_slots), and, on
     * the same stream, whatever the row's next sweep launches (slots that share a row share its stream: max_batch < URF_ASYNC_SLOTS).
     * The planes or staging rows it reads again belong to this slot resp. this row until then. */
    rc = auto_pass(c, sl.cap_a, sl.cap_dp, sl.cap_planned, st, 1u + (uint32_t)(&sl - c->slots), c->max_batch + (uint32_t)(&sl - c->slots), n_points);
    if (rc != URF_OK)
        return rc;
    URF_HIP(c, hipEventRecord(sl.ev_done, st));
    HT(3, ht0);
    sl.pending = true;
    sl.used = true;
    sl.n_points = n_points;
    sl.point_step = point_step;
    sl.off_x = off_x;
    sl.off_y = off_y;
    sl.off_z = off_z;
    sl.ticket = c->next_ticket;
    sl.out_bits = c->pol.sweep_outputs;   /* (it cannot change while the sweep is pending) */
    sl.out_direct = c->pol.sweep_direct;
    sl.gen = ++c->row_gen[slot_row(c, sl)];
    *ticket = c->next_ticket++;
    return URF_OK;
}

extern "C" int urf_classify_pc2_wait(urf_ctx* c, uint32_t ticket, uint8_t* labels_out, urf_scan_info* info)
{
    if (!c)
        return URF_ERR_INVALID_ARG;
    urf_ctx::slot_t& sl = c->slots[ticket % URF_ASYNC_SLOTS];
    if (!sl.pending || sl.ticket != ticket)
        return URF_ERR_INVALID_ARG;
    URF_HIP(c, hipSetDevice(c->device));
    HT_START;
    URF_HIP(c, hipEventSynchronize(sl.ev_done));
    HT(4, ht0);
    /* the short launch sequence left out something this sweep needed (urf_policy::plan): once more, with it --
     * the message is still in the slot's device buffer -- and from now on for every sweep (on_redo) */
    for (int tries = 0; c->pol.on_redo(sl.h_info.p->status); tries++) {
        if (tries == 6) {
            sl.pending = false;
            return URF_ERR_HIP;   /* (cannot happen: the full sequence raises none) */
        }
        c->n_rerun++;
        /* the rerun is the row's LATEST submission: with fewer rows than sweeps in flight a later sweep shares this row, and
         * what it left there is overwritten now -- its read-backs of the row must answer URF_ERR_BUSY, not this sweep's data */
        sl.gen = ++c->row_gen[slot_row(c, sl)];
        /* with the parameters and capture mode the sweep was submitted with (urf_set_params may have been called since),
         * behind whatever the context's stream still does with the row */
        int rc = order_row_after_main(c, slot_row(c, sl), slot_stream(c, sl));
        if (rc == URF_OK)
            rc = slot_launch(c, sl, sl.n_run, sl.point_step, sl.off_x, sl.off_y, sl.off_z, &sl.cap_dp, (int)sl.cap_a.capture);   /* (a padded sweep: pad and length word are still in place) */
        if (rc == URF_OK && hipStreamSynchronize(slot_stream(c, sl)) != hipSuccess) {
            c->last_error = "hipStreamSynchronize (rerun of a voided sweep)";
            rc = URF_ERR_HIP;
        }
        if (rc != URF_OK) {
            sl.pending = false;   /* the slot must not stay busy for ever */
            return rc;
        }
    }
    /* only now is the sweep "the last call": its scratch row stays untouched until the row (or a batch call) is used again */
    publish_last(c, URF_LAST_SWEEP, 1, sl.cap_a, sl.cap_dp, sl.cap_planned, slot_row(c, sl), sl.gen);
    c->last.sweep_n = sl.n_points;   /* (the readers answer for the caller's points, whatever length the sweep ran as) */
    if (labels_out)
        std::memcpy(labels_out, sl.h_labels.p, sl.n_points);
    if (info)
        *info = *sl.h_info.p;
    sl.pending = false;
    HT(5, ht0);
    return URF_OK;
}

extern "C" int urf_result_labels(urf_ctx* c, uint32_t ticket, const uint8_t** labels)
{
    if (!c || !labels)
        return URF_ERR_INVALID_ARG;
    *labels = nullptr;
    const urf_ctx::slot_t& sl = c->slots[ticket % URF_ASYNC_SLOTS];
    if (!sl.used || sl.ticket != ticket || !sl.h_labels.p)
        return URF_ERR_INVALID_ARG;   /* never issued, or its slot has been used again since */
    if (sl.pending)
        return URF_ERR_BUSY;          /* not waited for yet: the buffer is still being written */
    *labels = sl.h_labels.p;
    return URF_OK;
}

/* where the results of the sweep in this slot are: the buffer of the way it was submitted (the switch may have changed since) */
static const uint32_t* sweep_result_words(const urf_ctx::slot_t& sl) { return sl.out_direct ? sl.m_out.p : sl.h_out.p; }

/* the ticket's slot for urf_result_marker_points / urf_result_ordered_indices: urf_result_labels' rules, and the sweep was submitted with `bit` */
static int sweep_result_slot(urf_ctx* c, uint32_t ticket, uint32_t bit, const char* what, const urf_ctx::slot_t*& out)
{
    const urf_ctx::slot_t& sl = c->slots[ticket % URF_ASYNC_SLOTS];
    if (!sl.used || sl.ticket != ticket)
        return URF_ERR_INVALID_ARG;   /* never issued, or its slot has been used again since */
    if (sl.pending)
        return URF_ERR_BUSY;          /* not waited for yet: the buffer is still being written */
    if (!(sl.out_bits & bit) || !sweep_result_words(sl)) {
        c->last_error = std::string(what) + ": the sweep was submitted without " +
                        (bit == URF_SWEEP_OUT_ORDER ? "URF_SWEEP_OUT_ORDER" : "URF_SWEEP_OUT_MARKER_POINTS") + " (urf_set_sweep_outputs)";
        return URF_ERR_INVALID_ARG;
    }
    out = &sl;
    return URF_OK;
}

extern "C" int urf_result_marker_points(urf_ctx* c, uint32_t ticket, const float** pts, uint32_t* count)
{
    if (!c || !pts || !count)
        return URF_ERR_INVALID_ARG;
    *pts = nullptr;
    *count = 0;
    const urf_ctx::slot_t* sl = nullptr;
    const int rc = sweep_result_slot(c, ticket, URF_SWEEP_OUT_MARKER_POINTS, "urf_result_marker_points", sl);
    if (rc != URF_OK)
        return rc;
    const uint32_t* const words = sweep_result_words(*sl);
    *pts = (const float*)words;
    if (sl->h_info.p->status != URF_OK)
        return URF_OK;   /* nothing is published for such a sweep */
    const uint32_t n = words[URF_SWEEP_HDR_MCOUNT];
    if (n > URF_DEG_CELLS)
        return URF_ERR_HIP;
    *count = n;
    return URF_OK;
}

extern "C" int urf_result_ordered_indices(urf_ctx* c, uint32_t ticket, const uint32_t** road, const uint32_t** curb, const uint32_t** ring10,
                                          uint32_t counts[3])
{
    if (!c || !counts)
        return URF_ERR_INVALID_ARG;
    counts[0] = counts[1] = counts[2] = 0;
    for (const uint32_t** p : { road, curb, ring10 })
        if (p)
            *p = nullptr;
    const urf_ctx::slot_t* sl = nullptr;
    const int rc = sweep_result_slot(c, ticket, URF_SWEEP_OUT_ORDER, "urf_result_ordered_indices", sl);
    if (rc != URF_OK)
        return rc;
    const uint32_t* const words = sweep_result_words(*sl);
    const uint32_t* lists = words + URF_SWEEP_HDR;
    const uint32_t* h = words + URF_SWEEP_HDR_LCOUNTS;
    const bool ok = sl->h_info.p->status == URF_OK;
    if (ok && (h[0] > sl->n_points || h[1] > sl->n_points || h[2] > sl->n_points || (uint64_t)h[0] + h[1] > sl->n_points))
        return URF_ERR_HIP;
    /* three lists at a stride of the points the sweep ran as (urf_set_sweep_quantum: padded); a sweep submitted direct: back to back */
    const size_t at1 = sl->out_direct ? (ok ? h[0] : 0u) : sl->n_run, at2 = sl->out_direct ? (ok ? (size_t)h[0] + h[1] : 0u) : 2 * (size_t)sl->n_run;
    if (road)
        *road = lists;
    if (curb)
        *curb = lists + at1;
    if (ring10)
        *ring10 = lists + at2;
    if (!ok)
        return URF_OK;
    counts[0] = h[0];
    counts[1] = h[1];
    counts[2] = h[2];
    return URF_OK;
}

extern "C" int urf_classify_pc2(urf_ctx* c, const uint8_t* data, uint32_t n_points, uint32_t point_step,
                                uint32_t off_x, uint32_t off_y, uint32_t off_z, uint8_t* labels_out, urf_scan_info* info)
{
    if (!c || !data || !labels_out || !pc2_layout_ok(point_step, off_x, off_y, off_z))
        return URF_ERR_INVALID_ARG;   /* before any byte of the message is copied */
    if (n_points > c->max_points)
        return URF_ERR_CAPACITY;
    if (n_points == 0) {
        if (info) {
            std::memset(info, 0, sizeof(*info));
            info->status = URF_TOO_FEW_POINTS;
        }
        return URF_OK;
    }
    uint32_t ticket = 0;
    const int rc = urf_classify_pc2_async(c, data, n_points, point_step, off_x, off_y, off_z, &ticket);
    if (rc != URF_OK)
        return rc;
    return urf_classify_pc2_wait(c, ticket, labels_out, info);
}

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
    return scan < l.scans && l.a.labels ? &l : nullptr;   /* (no call yet: no scans) */
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
    if (l.a.front && !(need == URF_NEED_RING_ORDER && c->pol.front_outputs)) {
        /* the last call went through the fused front end (urf_front.hpp), which keeps no ring-sorted copies: once more on its row through
         * the general kernels, as a batch call with every repair kernel in the sequence (same inputs -- a batch caller's arrays must still
         * be alive, a sweep of the callback path is still in its slot's device buffer and its row has not been resubmitted (checked
         * above) --, same parameters, same labels), and the context stays with them: a caller that reads ring-sorted results pays for
         * them once, not per call.  Only the record's arguments and parameters change: a sweep stays the sweep it was.
         * With urf_set_front_outputs on, the entry points that only need the rings' points in order (URF_NEED_RING_ORDER) take the fused
         * call as it is: launch_ordered / launch_markers run the kernels of urf_k_front_outputs.hpp next to the general ones. */
        c->pol.set(c->pol.want_ring_sorted, true);
        rc = run_pipeline(c, urf_call{ l.a.x, l.a.y, l.a.z, l.a.offsets, l.a.n_per_scan, l.a.max_len, l.a.n_scans, l.a.labels, nullptr, l.row,
                                       nullptr, &l.dp, (int)l.a.capture, true }, l.a, l.dp);
        if (rc == URF_OK)
            l.planned = c->planned;
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
    const urf_kargs& a = l.a;
    const urf_dev_params& dp = l.dp;
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
    const urf_fx_call k = fx_call_of(a, dp, l.planned, rows, 0u);
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t* r = &rec[(size_t)s * URF_FX_WORDS];
        const urf_fx_scan v = urf_front_scan_rule(k, r, ok[s], ncand[s], info[s].status, lens[s]);   /* (the rule k_front_digest applies on the device) */
        urf_front_why w;
        std::memset(&w, 0, sizeof w);
        w.fused = v.fused;
        w.call = l.planned.call.why;
        w.advice = l.planned.call.advice | v.advice;
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

static int ensure_order_scratch(urf_ctx* c, uint32_t n_scans)
{
    const size_t n = (size_t)n_scans * c->sstride;
    int rc;
    if ((rc = grow(c, c->ord_keys, n, c->stream)) != URF_OK || (rc = grow(c, c->ord_pos, n, c->stream)) != URF_OK)
        return rc;
    return grow(c, c->ord_cls, (size_t)n_scans * URF_MAX_CHANNELS * 2, c->stream);
}

/* The pre-pass of the read-outs of a fused call (urf_k_front_outputs.hpp) for scans [s0, s0 + n) of the last call: scratch, then
 * k_front_out_prep unless the arrays already hold exactly that (same recorded call, same range). */
static int front_out_prepare(urf_ctx* c, const urf_last_call& l, uint32_t s0, uint32_t n)
{
    const size_t cnt = (size_t)n * c->sstride;
    const bool regrow = cnt > c->fo_az.cap || cnt > c->fo_ent.cap || cnt > c->fo_d.cap;
    int rc;
    if ((rc = grow(c, c->fo_az, cnt, c->stream)) != URF_OK || (rc = grow(c, c->fo_ent, cnt, c->stream)) != URF_OK ||
        (rc = grow(c, c->fo_d, cnt, c->stream)) != URF_OK) {
        c->fo_prep.seq = 0;
        return rc;
    }
    if (!regrow && c->fo_prep.seq == c->last_seq && c->fo_prep.s0 == s0 && c->fo_prep.n == n)
        return URF_OK;
    c->fo_prep.seq = 0;
    hipLaunchKernelGGL(k_front_out_prep, dim3(l.a.tiles, n), dim3(256), 0, c->stream, l.a, l.dp, s0, c->fo_az.p, c->fo_ent.p, c->fo_d.p);
    URF_HIP(c, hipGetLastError());   /* (the mark only behind a launch that was accepted) */
    c->fo_prep.seq = c->last_seq;
    c->fo_prep.s0 = s0;
    c->fo_prep.n = n;
    return URF_OK;
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
    const uint32_t WL = l.a.max_len, max_len = l.dense.max_len;   /* (the padded call's scans are W * L points each) */
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
    const urf_kargs& a = l.a;   /* the call's own arguments and parameters, whatever was set since */
    const urf_dev_params& dp = l.dp;
    const bool fused = a.front != 0;   /* (last_call: only with urf_set_front_outputs on) a scan is either kind's, decided on the device */
    int rc = ensure_order_scratch(c, n);
    if (rc == URF_OK && fused)
        rc = front_out_prepare(c, l, s0, n);
    if (rc != URF_OK)
        return rc;
    hipLaunchKernelGGL(k_ring_order, dim3((unsigned)dp.p.channels, n), dim3(256), (2 * (size_t)a.tiles + 1) * sizeof(unsigned), c->stream, a, dp,
                       s0, c->ord_keys.p, c->ord_pos.p, c->ord_cls.p);
    if (fused)
        hipLaunchKernelGGL(k_ring_order_front, dim3((unsigned)dp.p.channels, n), dim3(256), 0, c->stream, a, dp, s0, c->fo_az.p, c->fo_ent.p,
                           c->ord_pos.p, c->ord_cls.p);
    hipLaunchKernelGGL(k_ordered_lists, dim3((unsigned)dp.p.channels, n), dim3(256), 0, c->stream, a, dp, s0, c->ord_pos.p, c->ord_cls.p, d_road,
                       d_curb, d_r10, stride, d_counts);
    URF_HIP(c, hipGetLastError());
    return l.dense.on ? dense_unmap(c, l, s0, n, d_road, d_curb, d_r10, stride, d_counts) : URF_OK;   /* (refuse_dense: the switch is on) */
}

extern "C" int urf_ordered_indices_batch(urf_ctx* c, uint32_t* d_road, uint32_t* d_curb, uint32_t* d_ring10, uint32_t stride,
                                         uint32_t* d_counts)
{
    const urf_last_call* l = c ? last_valid(c) : nullptr;
    if (!l || !d_counts || refuse_dense(c, "urf_ordered_indices_batch", true) || stride < (l->dense.on ? l->dense.max_len : l->a.max_len))
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
    const uint32_t S = l->scans, max_len = dense ? l->dense.max_len : l->a.max_len, stride = max_len ? max_len : 1u;
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
    const urf_kargs& a = l->a;   /* (after a rerun: the same labels, inputs and offsets) */
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
    src.x = (const unsigned*)c->last.a.x;
    src.y = (const unsigned*)c->last.a.y;
    src.z = (const unsigned*)c->last.a.z;
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
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    int rc;
    if ((rc = grow(c, c->mk_d, n * cells, c->stream)) != URF_OK || (rc = grow(c, c->mk_pos, n * cells, c->stream)) != URF_OK ||
        (rc = grow(c, c->mk_red, n * (cells + URF_MAX_CHANNELS), c->stream)) != URF_OK)
        return rc;
    const urf_kargs& a = l.a;
    const urf_dev_params& dp = l.dp;
    const bool fused = a.front != 0;   /* (as in launch_ordered) */
    if (fused && (rc = front_out_prepare(c, l, s0, n)) != URF_OK)
        return rc;
    uint8_t* const mk_lit = c->mk_red.p + n * cells;
    hipLaunchKernelGGL(k_marker_ring, dim3((unsigned)dp.p.channels, n), dim3(256), (2 * (size_t)a.tiles + 1) * sizeof(unsigned), c->stream, a, dp, s0,
                       c->mk_d.p, c->mk_pos.p, c->mk_red.p, mk_lit);
    /* rings in which the ORDER of equal azimuths decides a marker point (normally none: every workgroup returns at once) */
    hipLaunchKernelGGL(k_marker_ring_literal, dim3((unsigned)dp.p.channels, n), dim3(256), 0, c->stream, a, dp, s0, mk_lit, c->mk_d.p, c->mk_pos.p, c->mk_red.p);
    if (fused) {
        hipLaunchKernelGGL(k_marker_ring_front, dim3((unsigned)dp.p.channels, n), dim3(256), 0, c->stream, a, dp, s0, c->fo_az.p, c->fo_ent.p,
                           c->fo_d.p, c->mk_d.p, c->mk_pos.p, c->mk_red.p, mk_lit);
        hipLaunchKernelGGL(k_marker_ring_literal_front, dim3((unsigned)dp.p.channels, n), dim3(256), 0, c->stream, a, dp, s0, mk_lit, c->fo_az.p,
                           c->fo_ent.p, c->fo_d.p, c->mk_d.p, c->mk_pos.p, c->mk_red.p);
    }
    hipLaunchKernelGGL(k_marker_bins, dim3(n), dim3(384), 0, c->stream, a, dp, s0, c->mk_d.p, c->mk_pos.p, c->mk_red.p, d_pts, d_counts);
    if (fused)
        hipLaunchKernelGGL(k_marker_bins_front, dim3(n), dim3(384), 0, c->stream, a, dp, s0, c->mk_d.p, c->mk_pos.p, c->mk_red.p, d_pts, d_counts);
    URF_HIP(c, hipGetLastError());
    return URF_OK;
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
    const urf_kargs& k = l.a;
    const unsigned C = (unsigned)l.dp.p.channels;
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
    const urf_kargs& k = l->a;   /* the arguments and parameters of the call whose results are read */
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
    const unsigned C = (unsigned)l->dp.p.channels;
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

/* Benchmark helper: the submit / collect loop of a C or C++ client of the callback path (a ROS node's
 * subscriber callback and publisher), timed natively -- `n_sweeps` messages (taken round robin from
 * `msgs`), at most `in_flight` of them submitted before the oldest is collected. */
extern "C" int urf_bench_callback_stream(urf_ctx* c, const uint8_t* const* msgs, uint32_t n_msgs, uint32_t n_points,
                                         uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                         uint32_t n_sweeps, uint32_t in_flight, int producer_pinned, uint8_t* labels_out,
                                         double* seconds)
{
    if (!c || !msgs || n_msgs == 0 || !seconds || in_flight == 0 || in_flight > URF_ASYNC_SLOTS)
        return URF_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < n_msgs; k++)
        if (!msgs[k])
            return URF_ERR_INVALID_ARG;
    const size_t bytes = (size_t)n_points * point_step;
    uint32_t tickets[URF_ASYNC_SLOTS];
    uint32_t head = 0, count = 0;   /* ring of tickets in flight */
    urf_scan_info info;
    struct timespec t0, t1;
    c->ht_on = getenv("URF_HOST_TIMES") != nullptr;
    for (double& v : c->ht)
        v = 0.0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    auto loop = [&]() -> int {
        for (uint32_t k = 0; k < n_sweeps; k++) {
            if (count == in_flight) {
                const int rc = urf_classify_pc2_wait(c, tickets[head], labels_out, &info);
                if (rc != URF_OK)
                    return rc;
                head = (head + 1) % URF_ASYNC_SLOTS;
                count--;
            }
            const uint8_t* data = msgs[k % n_msgs];
            if (producer_pinned) {   /* the producer fills the library's pinned buffer itself (each slot's once: producing the data is not what is timed) */
                uint8_t* pin = nullptr;
                const int rc = urf_pinned_input(c, bytes, &pin);
                if (rc != URF_OK)
                    return rc;
                if (k < URF_ASYNC_SLOTS)
                    std::memcpy(pin, data, bytes);
                data = pin;
            }
            uint32_t t = 0;
            const int rc = urf_classify_pc2_async(c, data, n_points, point_step, off_x, off_y, off_z, &t);
            if (rc != URF_OK)
                return rc;
            tickets[(head + count) % URF_ASYNC_SLOTS] = t;
            count++;
        }
        while (count) {
            const int rc = urf_classify_pc2_wait(c, tickets[head], labels_out, &info);
            if (rc != URF_OK)
                return rc;
            head = (head + 1) % URF_ASYNC_SLOTS;
            count--;
        }
        return URF_OK;
    };
    const int lrc = loop();
    if (lrc != URF_OK) {
        c->ht_on = false;   /* (every exit path: a later call must not pay for the clock reads) */
        return lrc;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    *seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    if (c->ht_on) {
        fprintf(stderr, "host us per sweep (pinned %d, in flight %u): total %.1f | stage+h2d %.1f order %.1f launch %.1f record %.1f wait %.1f rest-of-wait %.1f\n",
                producer_pinned, in_flight, 1e6 * *seconds / n_sweeps, 1e6 * c->ht[0] / n_sweeps, 1e6 * c->ht[1] / n_sweeps, 1e6 * c->ht[2] / n_sweeps,
                1e6 * c->ht[3] / n_sweeps, 1e6 * c->ht[4] / n_sweeps, 1e6 * c->ht[5] / n_sweeps);
        c->ht_on = false;
    }
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

