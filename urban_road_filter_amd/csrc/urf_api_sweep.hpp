/* urf_api_sweep.hpp -- the callback path of the host API: its setters and queries, submission, collection, the hooks build's benchmark
 * loop.  A section of urf_api.hip (one translation unit), included once behind run_pipeline and launch_readouts. */
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
    urf_readout_scratch& w = c->sweep_ro;
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
            *n_resident += sl.cache.resident(c->pol.epoch);
    }
    return URF_OK;
}

/* ---- the callback path: one sweep, host buffers ------------------------------- */
/* Slot i of the callback path works on scratch row i % rows, rows = min(max_batch, URF_ASYNC_SLOTS), and on
 * that row's compute stream (row 0: the context's stream): with a context created for several scans the
 * kernels of as many sweeps overlap on the device (a single sweep's kernels are a few dozen workgroups
 * each).  With max_batch == 1 all slots share row 0 and the context's stream: only the copies overlap. */
static uint32_t slot_row(const urf_ctx* c, const urf_ctx::slot_t& sl)
{
    return (uint32_t)(&sl - c->slots) % sweep_rows(c);
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
        sl.cache.invalidate();
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

/* urf_set_sweep_outputs: the read-outs of the sweep run_pipeline has just launched on `st`, behind it on the same stream (launch_readouts)
 * -- with the sweep's own arguments and parameters (sl.run: its scratch row, scan 0), the row's read-out scratch and the slot's result
 * buffers; then the copies to the slot's pinned buffer.  A fused sequence (run.a.front) always holds the pre-pass; a voided sweep leaves
 * empty results (every kernel returns for a status that is not URF_OK) until its rerun.  c->fo_prep is none of its business. */
static int sweep_outputs_launch(urf_ctx* c, urf_ctx::slot_t& sl, uint32_t row, hipStream_t st, uint32_t n_points)
{
    const uint32_t bits = c->pol.sweep_outputs;
    if (!bits)
        return URF_OK;
    const bool merged = bits == (URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER) && !(c->debug_flags & URF_DBG_SWEEP_OLD_KERNELS);
    /* urf_set_sweep_results_direct: the slot's mapped pinned buffer as the device sees it -- the last kernels of the chain store header
     * results and lists there themselves, the lists back to back (k_sweep_lists_direct / k_ordered_lists_direct), and nothing is copied */
    const bool direct = c->pol.sweep_direct;
    uint32_t* const out = direct ? sl.m_out.dev : sl.d_out.p;
    uint32_t* const d_road = out + URF_SWEEP_HDR;
    const urf_readout_dst dst{ d_road, d_road + n_points, d_road + 2 * (size_t)n_points, n_points, out + URF_SWEEP_HDR_LCOUNTS, (float*)out,
                               out + URF_SWEEP_HDR_MCOUNT };
    const int rc = launch_readouts(c, sl.run, st, 0u, 1u, c->sweep_ro.view(row, c->sstride), bits, sl.run.a.front != 0, merged, direct, dst);
    if (rc != URF_OK)
        return rc;
    if (direct)
        return URF_OK;   /* (the results are where the host reads them once the slot's event has completed) */
    URF_HIP(c, hipMemcpyAsync(sl.h_out.p, out, URF_SWEEP_HDR * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (bits & URF_SWEEP_OUT_ORDER)
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
    const int rc = run_pipeline(c, urf_call{ sx, sy, sz, nullptr, n_points, n_points, 1, sl.d_labels.p, nullptr, row, st, dp_in, capture_in }, sl.run);
    if (rc != URF_OK)
        return rc;
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

/* Stage: the message goes to the device on the slot's own stream, in front of the sweep's kernels.  (r2 / r3 used a copy
 * stream of its own and an event per sweep for the slot's stream to wait on: 7 870 -> 8 670 sweeps/s with a pinned
 * producer, 6 460 -> 7 540 staged without them.  The four streams still map to three hardware queues -- kernel
 * trace, profiles/r3_callback_trace_after.txt --, but more queues made things worse, see profiles/README.md.)
 * Sweeps of other slots run beside the copy as before. */
static int sweep_stage(urf_ctx* c, urf_ctx::slot_t& sl, hipStream_t st, const uint8_t* data, uint32_t n_points, uint32_t point_step,
                       uint32_t off_x, uint32_t off_y, uint32_t off_z, bool planes, const urf_sweep_dims& sh)
{
    if (planes) {
        /* gathered into the pinned planes (pc2_to_planes) in two halves, so that the first one is on its way while the
         * second one is gathered (one 2-D copy per half: its columns of the three planes; 35 us for the whole, 22 per
         * half).  (urf_pinned_input() lets a producer write its records into the pinned buffer directly: no staging.) */
        float* X = (float*)sl.h_in.p;
        const size_t n4 = ((size_t)sh.n_run + 3) & ~(size_t)3;
        const size_t real4 = ((size_t)n_points + 3) & ~(size_t)3;   /* (the halves are halves of the sweep's own points; no pad: n4) */
        const uint32_t mid = n_points >= 32768 ? (uint32_t)((real4 / 2) & ~(size_t)3) : 0u;
        const uint32_t cut[3] = { 0u, mid, n_points };
        for (int h = mid ? 0 : 1; h < 2; h++) {
            pc2_to_planes(data, cut[h], cut[h + 1], point_step, off_x, off_y, off_z, X, X + n4, X + 2 * n4);
            if (h == 1 && sh.n_run != n_points) {   /* the pad: the planes' tails, which the second copy's columns [mid, n_run) carry */
                const float nan = std::numeric_limits<float>::quiet_NaN();
                for (float* P : { X, X + n4, X + 2 * n4 })
                    std::fill(P + n_points, P + sh.n_run, nan);
            }
            const size_t w = (h == 1 ? n4 - cut[1] : cut[1]) * sizeof(float), o = cut[h] * sizeof(float);
            URF_HIP(c, hipMemcpy2DAsync(sl.d_raw.p + o, n4 * sizeof(float), sl.h_in.p + o, n4 * sizeof(float), w, 3, hipMemcpyHostToDevice, st));
        }
        return URF_OK;
    }
    URF_HIP(c, hipMemcpyAsync(sl.d_raw.p, sl.h_in.p, (size_t)n_points * point_step, hipMemcpyHostToDevice, st));
    if (sh.pad) {   /* the sweep's own length for k_pc2_to_soa_pad: a word of the slot, copied in front of every launch of the sequence */
        *sl.h_n.p = n_points;
        URF_HIP(c, hipMemcpyAsync(sl.d_n.p, sl.h_n.p, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    return URF_OK;
}

/* the slot's sequence for `key`, captured once and replayed; sl.run is what the sweep runs with either way (readers' record, rerun) */
static int sweep_sequence(urf_ctx* c, urf_ctx::slot_t& sl, hipStream_t st, const uint64_t key[3], uint32_t n_run, uint32_t point_step,
                          uint32_t off_x, uint32_t off_y, uint32_t off_z)
{
    bool hit;
    const unsigned at = sl.cache.acquire(key, c->pol.sweep_quantum ? URF_SWEEP_SEQS : 1u, hit, [&](unsigned i) { seq_drop(sl, i); });
    urf_ctx::slot_t::seq_t& q = sl.seqs[at];
    if (!hit) {
        seq_drop(sl, at);   /* (the entry that makes room, or what a failed instantiation left in a free one) */
        URF_HIP(c, hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
        const int rc = slot_launch(c, sl, n_run, point_step, off_x, off_y, off_z);
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(st, &g);
        if (rc != URF_OK || e != hipSuccess) {
            if (g)
                (void)hipGraphDestroy(g);
            if (rc == URF_OK)
                URF_HIP(c, e);
            return rc;
        }
        q.graph = g;
        URF_HIP(c, hipGraphInstantiate(&q.exec, q.graph, nullptr, nullptr, 0));
        sl.cache.take(at, key);
        q.run = sl.run;
        c->n_captured++;
    } else {
        sl.run = q.run;
    }
    sl.cache.e[at].used = ++c->seq_clock;
    URF_HIP(c, hipGraphLaunch(q.exec, st));
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
    HT_START;
    /* a message inside the slot's pinned buffer must be the buffer urf_pinned_input() handed out, and
     * fit it: a larger one would make slot_prepare() free the very memory it is about to read */
    if (sl.h_in.p && data >= sl.h_in.p && data < sl.h_in.p + sl.h_in.cap && (data != sl.h_in.p || (size_t)n_points * point_step > sl.h_in.cap))
        return URF_ERR_INVALID_ARG;
    const bool planes = data != sl.h_in.p;   /* (a producer that filled the pinned buffer itself wrote records) */
    const urf_sweep_dims sh = urf_sweep_shape(n_points, point_step, c->pol.sweep_quantum, c->max_points, planes, std::min(sl.h_in.cap, sl.d_raw.cap));
    int rc = slot_prepare(c, sl, sh.want);
    if (rc == URF_OK && !planes)
        rc = ensure_soa_staging(c);   /* where the device gathers the records' x / y / z */
    if (rc != URF_OK)
        return rc;
    hipStream_t st = slot_stream(c, sl);
    if ((rc = order_row_after_main(c, slot_row(c, sl), st)) != URF_OK ||
        (rc = sweep_stage(c, sl, st, data, n_points, point_step, off_x, off_y, off_z, planes, sh)) != URF_OK)
        return rc;
    if (planes != sl.planes)
        sl.cache.invalidate();   /* the captured sequences read the other format */
    sl.planes = planes;
    sl.n_run = sh.n_run;
    sl.pad = sh.pad;
    HT(0, ht0);   /* staging + H2D enqueue */
    /* what earlier calls reported, for this sweep and the replayed sequences (outside the stream capture: fold may synchronise) */
    rc = c->pol.fold(c, st);
    if (rc != URF_OK)
        return rc;
    c->pol.probation_sweep();
    if (c->pol.auto_on)   /* urf_set_front_auto: the sweep's advice, applied before its sequence is chosen (a change bumps the epoch) */
        auto_at_call(c, std::max<uint32_t>((sh.n_run + URF_TILE - 1) / URF_TILE, 1u), 1u, (uint32_t)c->capture, true);
    /* anything a captured sequence depends on bumps the epoch */
    const uint64_t key[3] = { c->pol.epoch, ((uint64_t)sh.n_run << 32) | point_step, ((uint64_t)off_x << 42) ^ ((uint64_t)off_y << 21) ^ off_z };
    const bool use_graph = !c->timing && !(c->debug_flags & 8u);
    HT(1, ht0);   /* event record, ordering, stream wait */
    rc = use_graph ? sweep_sequence(c, sl, st, key, sh.n_run, point_step, off_x, off_y, off_z)
                   : slot_launch(c, sl, sh.n_run, point_step, off_x, off_y, off_z);
    if (rc != URF_OK)
        return rc;
    HT(2, ht0);   /* graph launch (or the launches themselves) */
    /* urf_set_front_auto's learning pass: no part of the captured sequence, on the sweep's stream behind it and in front of ev_done --
     * the event urf_classify_pc2_wait waits for, the context's stream waits for before it touches a row (order_after_slots), and, on
     * the same stream, whatever the row's next sweep launches (slots that share a row share its stream: max_batch < URF_ASYNC_SLOTS).
     * The planes or staging rows it reads again belong to this slot resp. this row until then. */
    rc = auto_pass(c, sl.run, st, 1u + (uint32_t)(&sl - c->slots), c->max_batch + (uint32_t)(&sl - c->slots), n_points);
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
            rc = slot_launch(c, sl, sl.n_run, sl.point_step, sl.off_x, sl.off_y, sl.off_z, &sl.run.dp, (int)sl.run.a.capture);   /* (a padded sweep: pad and length word are still in place) */
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
    publish_last(c, URF_LAST_SWEEP, 1, sl.run, slot_row(c, sl), sl.gen);
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

#ifdef URF_ENABLE_TEST_HOOKS
/* Benchmark helper (include/urf_test_hooks.h: the hooks build only): the submit / collect loop of a C or C++ client of the callback
 * path (a ROS node's subscriber callback and publisher), timed natively -- `n_sweeps` messages (taken round robin from
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
#endif   /* URF_ENABLE_TEST_HOOKS */
