/* urf_ctx.hpp -- the context of the host API: its buffers, the scratch arrays declared once, urf_run, "the last call", the read-out scratch,
 * urf_ctx and its allocation helpers.  A section of urf_api.hip (one translation unit), included once behind the kernels' headers. */
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

/* "The last call", for the entry points that take their input from it (urf_read_stage, urf_ordered_indices, urf_marker_points,
 * urf_clouds_batch_*): publish_last() is the only writer of the whole record, last_call() the readers' way to it. */
enum urf_last_kind { URF_LAST_NONE, URF_LAST_SOA, URF_LAST_PC2, URF_LAST_SWEEP };   /* no call yet | the batch entry point | a sweep waited for */
/* plan()'s decision about a call in words, kept for urf_front_explain: the terms that were false and the advice (urf_policy::why), and
 * whether the march was, or would have been, the multi-sector one (ms_ok) */
struct urf_planned {
    urf_policy::reasons call = { 0u, 0u };
    bool ms = false;
};
/* what a call ran with (run_pipeline fills one; the last call, the sweep in a slot and each of a slot's captured sequences keep theirs) */
struct urf_run {
    urf_kargs a;
    urf_dev_params dp;
    urf_planned planned;
};
struct urf_last_call {
    int kind = URF_LAST_NONE;
    uint32_t scans = 0;
    urf_run run;                    /* what it ran with (urf_front_explain: run.planned) */
    uint32_t row = 0;               /* the scratch row of run.a.* (a batch call: 0) */
    uint64_t gen = 0;               /* a sweep: the row's submission number it was (urf_ctx::row_gen) */
    uint32_t sweep_n = 0;           /* a sweep: the caller's number of points (urf_set_sweep_quantum: run.a.n_per_scan is the padded length) */
    /* a dense call (urf_classify_batch_*_dense): `run.a` is the padded batch -- staging, padded labels, all the context's own --, and
     * this is what the caller handed in, for urf_clouds_batch_* in input order (offsets: the context's copy) */
    struct {
        bool on = false;
        const float *x = nullptr, *y = nullptr, *z = nullptr;   /* a SoA call's */
        uint8_t* labels = nullptr;
        uint32_t max_len = 0;
    } dense;
};

/* The scratch of the read-out chain (launch_readouts: published order and marker points), declared once and held twice: urf_ctx::ro,
 * which the batch read-backs grow per call, only what the call's products need; and urf_ctx::sweep_ro, the callback path's, of fixed
 * size, allocated whole by the setters (sweep_outputs_alloc).  A view is the nine pointers at a row: r * elements into each array. */
struct urf_readout_view {
    float *mk_d, *fo_d;
    uint32_t *mk_pos, *ord_pos, *ord_cls, *fo_az, *fo_ent;
    uint8_t* mk_red;
    unsigned long long* ord_keys;
};
struct urf_readout_scratch {
    lazy_buf<float> mk_d;               /* [rows][URF_MAX_CHANNELS * URF_DEG_CELLS] */
    lazy_buf<uint32_t> mk_pos;
    lazy_buf<uint8_t> mk_red;           /* ... + URF_MAX_CHANNELS literal flags behind the cells: of a row (sweep_ro), of all the call's scans (ro) */
    lazy_buf<unsigned long long> ord_keys;   /* [rows][sstride] */
    lazy_buf<uint32_t> ord_pos, ord_cls;     /* ord_cls: [rows][URF_MAX_CHANNELS][2] road / curb points per ring (k_ring_order -> k_ordered_lists) */
    /* a fused call's (k_front_out_prep): [rows][sstride] per ring-major position the azimuth's bits, input index | class << 30, planar distance */
    lazy_buf<uint32_t> fo_az, fo_ent;
    lazy_buf<float> fo_d;
    urf_readout_view view(size_t row, size_t sstride) const
    {
        const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
        return { mk_d.p + row * cells, fo_d.p + row * sstride, mk_pos.p + row * cells, ord_pos.p + row * sstride, ord_cls.p + row * URF_MAX_CHANNELS * 2,
                 fo_az.p + row * sstride, fo_ent.p + row * sstride, mk_red.p + row * (cells + URF_MAX_CHANNELS), ord_keys.p + row * sstride };
    }
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
        /* the captured sequences (with urf_set_sweep_quantum up to URF_SWEEP_SEQS): graph and run; live, key, last use: urf_seq_cache's */
        struct seq_t {
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            urf_run run;
        } seqs[URF_SWEEP_SEQS];
        urf_seq_cache cache;
        urf_run run;                    /* what the sweep in this slot ran with (its sequence's, or its direct launches') */
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
    /* urf_set_sweep_outputs: once per scratch row of the callback path, allocated by the first call that turns a bit on */
    urf_readout_scratch sweep_ro;
    bool streams_made = false;
    urf_policy pol;                 /* which kernels a call launches */
    uint32_t n_rerun = 0;           /* sweeps urf_classify_pc2_wait had to run again */
    uint32_t n_captured = 0;        /* launch sequences captured so far, all slots (urf_callback_path_captures) */
    uint64_t seq_clock = 0;         /* launches of captured sequences so far (urf_seq_cache: used) */
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
    /* the batch read-backs', sized for the most scans asked for so far; fo_prep: the recorded call's number and range of scans fo_* hold */
    urf_readout_scratch ro;
    struct { uint64_t seq = 0; uint32_t s0 = 0, n = 0; } fo_prep;
    uint64_t last_seq = 0;          /* bumped whenever `last` is written */
    lazy_buf<uint32_t> ord_lists;   /* single-scan entry point: 3 x sstride + 4 */
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
