/*
 * urf_k_outputs.hpp -- the outputs on demand: index lists, the published order, the road_marker points; the device self tests (test hooks).
 * One of the kernel families of urf_kernels.hpp (r6: split by family, zero behaviour change); included from there, in order.
 */
#ifndef URF_K_OUTPUTS_HPP
#define URF_K_OUTPUTS_HPP

/* A scan whose read-outs come from what the fused front end left on the device (urf_k_front_outputs.hpp, urf_set_front_outputs): the call was
 * fused (the host runs a fused call again through the general kernels unless that switch is on, and the record then says front == 0), the
 * scan kept its flag and has a result.  The kernels below that read ring-sorted copies return at once for such a scan, their siblings
 * for every other. */
__device__ __forceinline__ bool urf_scan_fused(const urf_kargs& a, unsigned s, const urf_scan_info& in)
{
    return a.front != 0u && in.status == URF_OK && a.front_ok[s] != 0u;
}

/* ------------------------------------------------------------------------- */
/* index lists                                                                 */
/* ------------------------------------------------------------------------- */
/* lidar_segmentation.cpp:354-367, 605-608, 620 as index sets: for every scan of a batch the
 * ascending lists of the input indices of its road / curb / roi / road_probably points.
 * Workgroup (t, s) = tile t (2048 labels) of scan s.  k_compact_count: the tile's four counts;
 * k_compact_write: the tile's first position in each list = the counts of the tiles before it, then
 * ranks inside the tile by ballot + prefix, eight rounds of 256 labels (ascending order kept). */
#define URF_COMPACT_THREADS 256
__device__ __forceinline__ unsigned urf_label_classes(unsigned l)
{
    return ((l & URF_LABEL_MASK) == URF_LABEL_ROAD ? 1u : 0u) | ((l & URF_LABEL_MASK) == URF_LABEL_CURB ? 2u : 0u) |
           ((l & URF_FLAG_ROI) ? 4u : 0u) | ((l & URF_FLAG_RING10) ? 8u : 0u);
}
__global__ __launch_bounds__(URF_COMPACT_THREADS) void k_compact_count(const uint8_t* __restrict__ labels, unsigned n_per_scan,
                                                                         unsigned tiles, unsigned* __restrict__ tile_cnt)
{
    __shared__ unsigned sh[4];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const uint8_t* L = labels + (size_t)s * n_per_scan;
    if (tid < 4)
        sh[tid] = 0;
    __syncthreads();
    unsigned c[4] = { 0, 0, 0, 0 };
    for (unsigned r = 0; r < URF_TILE / URF_COMPACT_THREADS; r++) {
        const unsigned i = t * URF_TILE + r * URF_COMPACT_THREADS + tid;
        const unsigned f = i < n_per_scan ? urf_label_classes(L[i]) : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++)
            c[k] += (unsigned)__popcll(__ballot((f >> k) & 1u));
    }
    if (urf_lane() == 0)
#pragma unroll
        for (int k = 0; k < 4; k++)
            atomicAdd(&sh[k], c[k]);
    __syncthreads();
    if (tid < 4)
        tile_cnt[((size_t)s * tiles + t) * 4 + tid] = sh[tid];
}
__global__ __launch_bounds__(URF_COMPACT_THREADS) void k_compact_write(const uint8_t* __restrict__ labels, unsigned n_per_scan,
                                                                         unsigned tiles, const unsigned* __restrict__ tile_cnt,
                                                                         unsigned* road, unsigned* curb, unsigned* roi,
                                                                         unsigned* ring10, unsigned* counts)
{
    __shared__ unsigned run[4], wsum[4][URF_COMPACT_THREADS / 64];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* L = labels + (size_t)s * n_per_scan;
    if (tid < 64) {   /* the tiles before this one: lane k + 4 j sums every 16th tile of class k */
        const unsigned k = tid & 3u;
        unsigned sum = 0;
        for (unsigned u = tid >> 2; u < t; u += 16)
            sum += tile_cnt[((size_t)s * tiles + u) * 4 + k];
        sum += __shfl_xor(sum, 4);
        sum += __shfl_xor(sum, 8);
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if (tid < 4)
            run[tid] = sum;
    }
    __syncthreads();
    unsigned* outs[4] = { road, curb, roi, ring10 };
    for (unsigned r = 0; r < URF_TILE / URF_COMPACT_THREADS; r++) {
        const unsigned i = t * URF_TILE + r * URF_COMPACT_THREADS + tid;
        const unsigned f = i < n_per_scan ? urf_label_classes(L[i]) : 0u;
        unsigned below[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long m = __ballot((f >> k) & 1u);
            below[k] = urf_popc_below(m);
            if (lane == 0)
                wsum[k][wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned pre = run[k];
            for (unsigned w = 0; w < wave; w++)
                pre += wsum[k][w];
            if (((f >> k) & 1u) && outs[k])
                outs[k][(size_t)s * n_per_scan + pre + below[k]] = i;
        }
        __syncthreads();
        if (tid < 4)
            run[tid] += wsum[tid][0] + wsum[tid][1] + wsum[tid][2] + wsum[tid][3];
        __syncthreads();
    }
    if (t + 1 == tiles && tid < 4 && counts)
        counts[(size_t)s * 4 + tid] = run[tid];
}

/* ------------------------------------------------------------------------- */
/* published order                                                             */
/* ------------------------------------------------------------------------- */
/* The reference sorts every ring by azimuth (lidar_segmentation.cpp:70-93, 289-291) and fills
 * its road / curb / road_probably clouds ring by ring in that order (:354-367, 605-608).  The
 * labels do not need that sort; callers that want the clouds in the reference's order do.
 * k_ring_order: one workgroup per ring of ONE scan sorts (azimuth bits, position in the ring)
 * and writes the ring-major position of the i-th point of the ring in azimuth order; a ring in
 * which two points share their azimuth bit for bit is then sorted AGAIN, literally as the
 * reference's Lomuto quicksort does it, whose order of equal azimuths is what gets published
 * (r5).  Rings of up to 2048 points sort in LDS, longer ones in global memory. */
/* What the per-ring read-out kernels write, per scan of the launch (blockIdx.y): the published order (sstride keys and entries, the ring's
 * road / curb counts) and the marker tables (URF_MAX_CHANNELS x URF_DEG_CELLS cells, one literal flag per ring).  A kernel that does not
 * produce a product leaves its pointers null. */
struct urf_ring_outs {
    unsigned long long* gkeys_all;
    unsigned* rord_all;
    unsigned* rcls_all;
    float* m_d_all;
    unsigned* m_pos_all;
    uint8_t* m_red_all;
    uint8_t* m_lit_all;
};

/* What is published for the ring's points, by position, staged in LDS by the instance that has label and source index of every point in
 * registers anyway (k_sweep_rings): urf_ring_publish reads it instead of two dependent loads per point. */
struct urf_ring_staged {
    const unsigned* ent;
    __device__ __forceinline__ unsigned at(unsigned i) const { return i; }
    __device__ __forceinline__ unsigned entry(unsigned i, unsigned& cls) const
    {
        const unsigned e = ent[i];
        cls = e >> 30;
        return e;
    }
};

/* One workgroup (256 threads) per ring of a scan with ring-sorted copies, for either product or both: ORDER, the ring's published order
 * (k_ring_order); MARK, its two marker tables (k_marker_ring); both, k_sweep_rings -- the ring's run table goes into LDS once, every
 * point's slot, coordinates, source index, label and exact azimuth are fetched and worked out once.
 *
 * The usual ring (at most 2048 points): every point is looked at ONCE -- its slot through the ring's run table in LDS (k_ring's map)
 * instead of a bisection in global memory, slot records, then labels, eight points per thread in flight at a time -- and azimuth, label
 * and slot stay in registers for the three marker passes and the sort's keys.  (Pass by pass, with seven dependent loads per point and
 * the exact azimuth worked out three times, k_marker_ring took longer than the whole classification: 3.9 ms per 1024 sweeps.)  The
 * marker passes here are the one deliberate specialisation of the rules of urf_marker_passes (urf_k_readouts.hpp): a change there is a
 * change here.  Longer rings, and for the published order rings with NaN azimuths, take the shared bodies of urf_k_readouts.hpp. */
template <bool ORDER, bool MARK>
__device__ __forceinline__ void urf_ring_readout(const urf_kargs& a, const urf_dev_params& dp, unsigned s0, const urf_ring_outs& o)
{
    constexpr unsigned NT = 256, NB = 2048, EPT = 8, CAP = NT * EPT;
    constexpr bool BOTH = ORDER && MARK;
    __shared__ unsigned long long A[ORDER ? CAP : 1];
    __shared__ unsigned cnt[ORDER ? URF_BLOCK_CNT(NB, NT) : 1];
    __shared__ urf_sort_shared ssh;
    __shared__ unsigned ncls[2], sh_tie;
    __shared__ int lom_stk[ORDER ? 2 * 64 : 1];
    __shared__ urf_marker_tabs T;
    __shared__ unsigned need_lit;   /* the ring's order decides (k_marker_ring_literal) */
    __shared__ unsigned staged[BOTH ? CAP : 1];
    extern __shared__ unsigned sh_ring_tab[];   /* P[tiles + 1], radd[tiles] (urf_ring_map) */
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;   /* per scan of the launch */
    unsigned* const rcls = ORDER ? o.rcls_all + ((size_t)blockIdx.y * URF_MAX_CHANNELS + c) * 2 : nullptr;   /* road / curb points of the ring */
    uint8_t* const m_lit = MARK ? o.m_lit_all + (size_t)blockIdx.y * URF_MAX_CHANNELS + c : nullptr;
    const urf_scan_info in = a.info[s];
    if (urf_scan_fused(a, s, in))
        return;   /* (uniform) k_ring_order_front's, k_marker_ring_front's */
    if (in.status != URF_OK || c >= in.n_rings) {
        if (ORDER && tid < 2)
            rcls[tid] = 0;
        if (MARK && tid == 0)
            *m_lit = 0;
        return;
    }
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned rel = ORDER ? a.ring_off[(size_t)s * (C + 1) + c] : 0u;   /* scan-relative start of the ring */
    const unsigned sb = urf_sbase(a, s);
    const unsigned ntiles = (len + URF_TILE - 1) / URF_TILE;
    const bool in_lds = n <= CAP;
    /* the ring's run table in LDS (k_ring's map): position in the ring -> ring-sorted slot without a bisection in global memory
     * (k_marker_ring alone keeps that bisection for its long rings) */
    unsigned* const mapP = sh_ring_tab;
    unsigned* const mapA = sh_ring_tab + a.tiles + 1;
    if (ORDER || in_lds) {
        const unsigned* gp = a.rpre + ((size_t)s * C + c) * (a.tiles + 1);
        const uint16_t* gs = a.rstart + ((size_t)s * C + c) * a.tiles;
        for (unsigned t = tid; t <= ntiles; t += NT) {
            const unsigned pt = gp[t];
            mapP[t] = pt;
            if (t < ntiles)
                mapA[t] = t * URF_TILE + gs[t] - pt;   /* relative to the scan's scratch base */
        }
    }
    if constexpr (ORDER) {
        if (tid < 2)
            ncls[tid] = 0;
        if (tid == 0)
            sh_tie = 0;
    }
    if constexpr (MARK) {
        T.init(tid);
        if (tid == 0)
            need_lit = 0;
    }
    __syncthreads();
    const urf_ring_map map = { mapP, mapA, ntiles, (float)ntiles / (float)(n > 0 ? n : 1) };
    const urf_ring_sorted v = { a, s, C, c, ntiles, sb, off, &map };
    /* bit-equal azimuths (urf_ring_literal_order): the keys go back into bucket order in the ring's stretch of wsg */
    volatile unsigned long long* const LIT = (volatile unsigned long long*)(a.wsg + sb + rel);
    /* (uniform) a ring with NaN azimuths: k_nan_rings ran the reference's quicksort literally and left the ring in its final order --
     * where a NaN lands is no function of the azimuths */
    const bool nan_ring = ORDER && ((a.nan_mask[(size_t)s * 4 + (c >> 5)] >> (c & 31u)) & 1u) != 0u;
    unsigned my_road = 0, my_curb = 0;
    if (in_lds && !nan_ring) {
        unsigned slot[EPT], sr[EPT];
        float az[EPT], px[EPT], py[EPT];
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {   /* coordinates of the thread's eight points in flight together */
            const unsigned p = tid + e * NT;
            slot[e] = p < n ? map.at(p) : 0u;
            if constexpr (MARK)
                sr[e] = a.rec[sb + slot[e]] & URF_REC_SRC_MASK;
            px[e] = a.rx[sb + slot[e]];
            py[e] = a.ry[sb + slot[e]];
        }
        unsigned labs = 0;   /* two bits per point */
        if constexpr (MARK) {
#pragma unroll
            for (unsigned e = 0; e < EPT; e++) {
                const unsigned src = (slot[e] & ~(URF_TILE - 1u)) + sr[e];
                const unsigned lab = a.labels[off + src] & URF_LABEL_MASK;
                labs |= lab << (2 * e);
                if (BOTH && tid + e * NT < n)
                    staged[tid + e * NT] = src | (lab << 30);   /* (urf_ring_sorted::entry) */
            }
        }
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {   /* (the slot's record holds an approximation of the azimuth: the published order and the tables are those of the exact one) */
            float d2;
            az[e] = urf_azimuth(px[e], py[e], &d2);
        }
        if constexpr (MARK) {
            /* pass 1: where does the scan of this ring stop in each degree (:318) */
            int bin[EPT];
#pragma unroll
            for (unsigned e = 0; e < EPT; e++) {
                bin[e] = urf_deg_bin(az[e]);
                if (tid + e * NT < n && az[e] == az[e] && ((labs >> (2 * e)) & 3u) != URF_LABEL_ROAD)
                    atomicMin(&T.nrmin[bin[e]], (int)urf_fbits(az[e]));
            }
            __syncthreads();
            /* pass 2: farthest road point in front of it (:325-335); key = (d, first in azimuth order) */
            unsigned long long mkey[EPT];
#pragma unroll
            for (unsigned e = 0; e < EPT; e++) {
                mkey[e] = 0;
                const bool road = tid + e * NT < n && az[e] == az[e] && ((labs >> (2 * e)) & 3u) == URF_LABEL_ROAD;
                if (road && (int)urf_fbits(az[e]) == T.nrmin[bin[e]])
                    need_lit = 1u;   /* the very azimuth of the degree's first non-road point: in front of it or behind? */
                if (road && (int)urf_fbits(az[e]) < T.nrmin[bin[e]]) {
                    const float x = px[e], y = py[e];
                    const float d = (float)__builtin_sqrt((double)(0.f - x) * (double)(0.f - x) + (double)(0.f - y) * (double)(0.f - y));
                    if (d > 0.0f) {   /* "d > maxDistanceRoad" with maxDistanceRoad starting at 0 */
                        mkey[e] = ((unsigned long long)urf_fbits(d) << 32) | (0xffffffffu - urf_fbits(az[e]));
                        atomicMax(&T.best[bin[e]], mkey[e]);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (unsigned e = 0; e < EPT; e++)
                if (mkey[e] != 0 && mkey[e] == T.best[bin[e]])
                    if (atomicMin(&T.bestpos[bin[e]], tid + e * NT) != 0xffffffffu)
                        need_lit = 1u;   /* two road points with this distance AND azimuth: which comes first? */
            __syncthreads();
            if (tid == 0)
                *m_lit = (uint8_t)need_lit;
            T.store(v, c, o.m_d_all + blockIdx.y * cells, o.m_pos_all + blockIdx.y * cells, o.m_red_all + blockIdx.y * cells, tid);
        }
        if constexpr (ORDER) {
            unsigned* const rord = o.rord_all + (size_t)blockIdx.y * a.sstride;   /* per scan of the launch: sstride entries */
            unsigned long long key[EPT];
#pragma unroll
            for (unsigned e = 0; e < EPT; e++) {
                const unsigned i = tid + e * NT;
                key[e] = i < n ? ((unsigned long long)urf_fbits(az[e]) << 32) | i : ~0ull;
            }
            urf_block_sort_keys<NT, EPT, NB>(key, n, A, cnt, &ssh, false);
            const bool lit = urf_ring_literal_order<NT>(v, n, A, LIT, &sh_tie, lom_stk, tid);
#pragma unroll
            for (unsigned e = 0; e < EPT; e++) {
                const unsigned j = tid + e * NT;
                if (j < n) {
                    const unsigned pos = lit ? (unsigned)LIT[j] : (unsigned)A[j];
                    if constexpr (BOTH)
                        urf_ring_publish(urf_ring_staged{ staged }, pos, &rord[rel + j], my_road, my_curb);
                    else
                        urf_ring_publish(v, pos, &rord[rel + j], my_road, my_curb);
                }
            }
        }
    } else {
        if constexpr (ORDER) {
            unsigned long long* const gkeys = o.gkeys_all + (size_t)blockIdx.y * a.sstride;
            unsigned* const rord = o.rord_all + (size_t)blockIdx.y * a.sstride;
            if (nan_ring) {
                for (unsigned j = tid; j < n; j += NT)
                    urf_ring_publish(v, a.ssrt[sb + rel + j], &rord[rel + j], my_road, my_curb);
            } else
                urf_ring_order_long<NT>(v, n, gkeys + rel, LIT, &sh_tie, lom_stk, rord + rel, my_road, my_curb, tid);
        }
        if constexpr (MARK) {
            if constexpr (ORDER) {
                urf_marker_passes(v, n, T, &need_lit, tid);
                if (tid == 0)
                    *m_lit = (uint8_t)need_lit;
                T.store(v, c, o.m_d_all + blockIdx.y * cells, o.m_pos_all + blockIdx.y * cells, o.m_red_all + blockIdx.y * cells, tid);
            } else {
                const urf_ring_sorted vg = { a, s, C, c, ntiles, sb, off, nullptr };
                urf_marker_passes(vg, n, T, &need_lit, tid);
                if (tid == 0)
                    *m_lit = (uint8_t)need_lit;
                T.store(vg, c, o.m_d_all + blockIdx.y * cells, o.m_pos_all + blockIdx.y * cells, o.m_red_all + blockIdx.y * cells, tid);
            }
        }
    }
    if constexpr (ORDER)
        urf_ring_publish_counts(my_road, my_curb, ncls, rcls, tid);
}

__global__ __launch_bounds__(256) void k_ring_order(urf_kargs a, urf_dev_params dp, unsigned s0,
                                                    unsigned long long* gkeys_all, unsigned* rord_all, unsigned* rcls_all)
{
    urf_ring_readout<true, false>(a, dp, s0, urf_ring_outs{ gkeys_all, rord_all, rcls_all, nullptr, nullptr, nullptr, nullptr });
}

/* The lists of one scan = its rings in order, every ring in azimuth order (k_ring_order left, per ring
 * position, the point's input index and class, and per ring the number of road / curb points): workgroup
 * (ring, scan) finds where its ring starts in each list (the counts of the rings in front of it) and
 * appends its points in order -- ballot + prefix per 256 entries.  (One workgroup per SCAN walking all
 * ring points with three barriers per 1024 of them took 1.5 ms per 1024 sweeps.)
 *
 * PACKED (urf_set_sweep_results_direct; one scan per launch): the three lists lie back to back in ONE area at road_all -- road [0, c0), curb
 * [c0, c0 + c1), road_probably [c0 + c1, c0 + c1 + c2) -- whatever the scan's length: every workgroup sums the road / curb counts of ALL
 * the scan's rings (at most 128 pairs, beside the sums of the rings in front of it) and has the bases of curb and road_probably from
 * that; `stride` is not read.  The area and the counts may be pinned host memory mapped into the device's address space: every word is
 * written once, with a plain store, by the thread that writes it in the strided layout, and nothing is read back or updated atomically. */
template <unsigned NT, bool PACKED = false>   /* threads of the workgroup */
__device__ __forceinline__ void urf_ordered_lists(const urf_kargs& a, const urf_dev_params& dp, unsigned s0, const unsigned* rord_all,
                                                  const unsigned* rcls_all, unsigned* road_all, unsigned* curb_all, unsigned* ring10_all,
                                                  unsigned stride, unsigned* counts_all)
{
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y;
    const unsigned* rord = rord_all + (size_t)blockIdx.y * a.sstride;
    const unsigned* rcls = rcls_all + (size_t)blockIdx.y * URF_MAX_CHANNELS * 2;
    unsigned* road = PACKED ? road_all : road_all ? road_all + (size_t)blockIdx.y * stride : nullptr;
    unsigned* curb = PACKED ? nullptr : curb_all ? curb_all + (size_t)blockIdx.y * stride : nullptr;       /* (PACKED: below) */
    unsigned* ring10 = PACKED ? nullptr : ring10_all ? ring10_all + (size_t)blockIdx.y * stride : nullptr;
    unsigned* counts = counts_all + (size_t)blockIdx.y * 3;
    __shared__ unsigned wsum[2][NT / 64];
    __shared__ unsigned base[2];
    __shared__ unsigned total[PACKED ? 2 : 1];
    static_assert(!PACKED || NT >= URF_MAX_CHANNELS, "one thread per ring sums the scan's counts");
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const urf_scan_info in = a.info[s];
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned nR = in.status == URF_OK ? in.n_rings : 0;
    if (c >= nR) {
        if (c == 0 && tid < 3)
            counts[tid] = 0;   /* nothing is published for this scan */
        return;
    }
    if (tid < 2)
        base[tid] = 0;
    if constexpr (PACKED) {
        if (tid < 2)
            total[tid] = 0;
    }
    __syncthreads();
    if constexpr (PACKED) {
        if (tid < nR) {   /* every ring of the scan; those in front of this one into base as well */
            const unsigned r0 = rcls[2 * tid], r1 = rcls[2 * tid + 1];
            atomicAdd(&total[0], r0);
            atomicAdd(&total[1], r1);
            if (tid < c) {
                atomicAdd(&base[0], r0);
                atomicAdd(&base[1], r1);
            }
        }
    } else if (tid < c) {   /* c <= 127 rings in front */
        atomicAdd(&base[0], rcls[2 * tid]);
        atomicAdd(&base[1], rcls[2 * tid + 1]);
    }
    __syncthreads();
    if constexpr (PACKED) {
        curb = road + total[0];
        ring10 = curb + total[1];
    }
    unsigned run0 = base[0], run1 = base[1];
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    for (unsigned j0 = 0; j0 < n; j0 += NT) {
        const unsigned j = j0 + tid;
        const unsigned ent = j < n ? rord[rel + j] : 0u;
        const unsigned src = ent & 0x3fffffffu, cls = j < n ? ent >> 30 : 0u;
        const unsigned long long m0 = __ballot(cls == URF_LABEL_ROAD), m1 = __ballot(cls == URF_LABEL_CURB);
        if (lane == 0) {
            wsum[0][wave] = (unsigned)__popcll(m0);
            wsum[1][wave] = (unsigned)__popcll(m1);
        }
        __syncthreads();
        unsigned p0 = run0 + urf_popc_below(m0), p1 = run1 + urf_popc_below(m1);
#pragma unroll
        for (unsigned w = 0; w < NT / 64; w++) {
            p0 += w < wave ? wsum[0][w] : 0u;
            p1 += w < wave ? wsum[1][w] : 0u;
            run0 += wsum[0][w];
            run1 += wsum[1][w];
        }
        if (cls == URF_LABEL_ROAD && road)
            road[p0] = src;
        if (cls == URF_LABEL_CURB && curb)
            curb[p1] = src;
        if (c == 10 && j < n && ring10)   /* lidar_segmentation.cpp:605-608: every point of sorted ring 10 */
            ring10[j] = src;
        __syncthreads();
    }
    if (tid == 0) {
        if (c + 1 == nR) {
            counts[0] = run0;
            counts[1] = run1;
            if (nR <= 10)
                counts[2] = 0;
        }
        if (c == 10)
            counts[2] = n;
    }
}
__global__ __launch_bounds__(256) void k_ordered_lists(urf_kargs a, urf_dev_params dp, unsigned s0, const unsigned* rord_all,
                                                       const unsigned* rcls_all, unsigned* road_all, unsigned* curb_all,
                                                       unsigned* ring10_all, unsigned stride, unsigned* counts_all)
{
    urf_ordered_lists<256>(a, dp, s0, rord_all, rcls_all, road_all, curb_all, ring10_all, stride, counts_all);
}
/* ... with the packed layout, for the one scan of a sweep (urf_set_sweep_results_direct with URF_SWEEP_OUT_ORDER alone, or with the kernels of
 * each product launched one by one): `area` holds all three lists, `counts` their three lengths */
__global__ __launch_bounds__(256) void k_ordered_lists_direct(urf_kargs a, urf_dev_params dp, const unsigned* rord, const unsigned* rcls,
                                                              unsigned* area, unsigned* counts)
{
    urf_ordered_lists<256, true>(a, dp, 0u, rord, rcls, area, nullptr, nullptr, 0u, counts);
}

/* ------------------------------------------------------------------------- */
/* road_marker: marker points                                                  */
/* ------------------------------------------------------------------------- */
/* lidar_segmentation.cpp:305-351 scans, for every integer degree, all rings in order and every ring
 * in ascending azimuth, remembers the farthest road point of that degree and stops at the first point
 * of that degree that is not road.  Per ring and degree that is: the smallest azimuth of a non-road
 * point (where the scan of this ring stops, and with it the whole scan), and the farthest road point
 * in front of it (ties: the first in azimuth order).  k_marker_ring builds these two tables per ring
 * in LDS (urf_marker_tabs; no sort needed), k_marker_bins walks the rings per degree. */
__global__ __launch_bounds__(256) void k_marker_ring(urf_kargs a, urf_dev_params dp, unsigned s0,
                                                     float* m_d_all, unsigned* m_pos_all, uint8_t* m_red_all, uint8_t* m_lit_all)
{
    urf_ring_readout<false, true>(a, dp, s0, urf_ring_outs{ nullptr, nullptr, nullptr, m_d_all, m_pos_all, m_red_all, m_lit_all });
}

/* Both products of a sweep of the callback path in one launch (urf_set_sweep_outputs with both bits): grid (channels, 1).  k_marker_ring_literal
 * follows it as it follows k_marker_ring. */
__global__ __launch_bounds__(256) void k_sweep_rings(urf_kargs a, urf_dev_params dp, urf_ring_outs o)
{
    urf_ring_readout<true, true>(a, dp, 0u, o);
}

/* The same tables when the ring's ORDER decides (urf_marker_literal).  k_marker_ring flags such a ring (m_lit); this kernel, launched
 * behind it on the same grid, returns at once for every other ring. */
__global__ __launch_bounds__(256) void k_marker_ring_literal(urf_kargs a, urf_dev_params dp, unsigned s0, const uint8_t* m_lit_all,
                                                             float* m_d_all, unsigned* m_pos_all, uint8_t* m_red_all)
{
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    if (urf_scan_fused(a, s, a.info[s]))
        return;   /* (uniform) k_marker_ring_literal_front's; its flag is not written yet */
    if (!m_lit_all[(size_t)blockIdx.y * URF_MAX_CHANNELS + c])
        return;
    __shared__ urf_marker_tabs T;
    __shared__ int stk[2 * 64];
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned sb = urf_sbase(a, s);
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    const urf_ring_sorted v = { a, s, C, c, (len + URF_TILE - 1) / URF_TILE, sb, off, nullptr };
    urf_marker_literal(v, n, (volatile unsigned long long*)(a.wsg + sb + rel), T, stk, tid);
    T.store(v, c, m_d_all + blockIdx.y * cells, m_pos_all + blockIdx.y * cells, m_red_all + blockIdx.y * cells, tid);
}

__global__ __launch_bounds__(384) void k_marker_bins(urf_kargs a, urf_dev_params dp, unsigned s0, const float* m_d_all,
                                                     const unsigned* m_pos_all, const uint8_t* m_red_all, float* out_all,
                                                     unsigned* count_all)
{
    __shared__ unsigned wsum[6];
    const unsigned s = s0 + blockIdx.x;
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    const urf_scan_info in = a.info[s];
    if (urf_scan_fused(a, s, in))
        return;   /* (uniform) k_marker_bins_front's */
    urf_marker_bins<urf_ring_sorted>(a, 0u, in.status == URF_OK ? in.n_rings : 0, m_d_all + blockIdx.x * cells, m_pos_all + blockIdx.x * cells,
                                     m_red_all + blockIdx.x * cells, out_all + (size_t)blockIdx.x * URF_DEG_CELLS * 4, count_all + blockIdx.x,
                                     wsum);
}

/* k_ordered_lists and k_marker_bins depend on nothing of each other: for ONE sweep of the callback path (urf_set_sweep_outputs with both
 * bits) they are one launch, grid (channels + 1, 1) x 384 threads -- workgroups 0 .. channels - 1 append their ring to the lists,
 * workgroup `channels` walks the rings' marker tables per degree, for a scan of either kind (urf_scan_fused: k_marker_bins_front's view). */
struct urf_sweep_lists_args {
    const unsigned *rord, *rcls;
    unsigned *road, *curb, *ring10, *list_counts;   /* lists of `stride` entries, 3 counts */
    unsigned stride;
    const float* m_d;
    const unsigned* m_pos;
    const uint8_t* m_red;
    float* pts;            /* URF_DEG_CELLS x 4 */
    unsigned* pts_count;
};
/* the last workgroup of such a launch: the marker points of the sweep's one scan, of either kind */
__device__ __forceinline__ void urf_sweep_marker_bins(const urf_kargs& a, const urf_sweep_lists_args& o)
{
    __shared__ unsigned wsum[6];
    const urf_scan_info in = a.info[0];
    if (urf_scan_fused(a, 0u, in)) {
        unsigned off, len;
        urf_scan_range(a, 0u, off, len);
        urf_marker_bins<urf_ring_fused>(a, off, in.n_rings, o.m_d, o.m_pos, o.m_red, o.pts, o.pts_count, wsum);
    } else
        urf_marker_bins<urf_ring_sorted>(a, 0u, in.status == URF_OK ? in.n_rings : 0, o.m_d, o.m_pos, o.m_red, o.pts, o.pts_count, wsum);
}
__global__ __launch_bounds__(384) void k_sweep_lists(urf_kargs a, urf_dev_params dp, urf_sweep_lists_args o)
{
    if (blockIdx.x < (unsigned)dp.p.channels) {   /* (uniform) */
        urf_ordered_lists<384>(a, dp, 0u, o.rord, o.rcls, o.road, o.curb, o.ring10, o.stride, o.list_counts);
        return;
    }
    urf_sweep_marker_bins(a, o);
}

/* k_sweep_lists with the packed list layout (urf_set_sweep_results_direct): o.road is the list area, o.curb, o.ring10 and o.stride are
 * not read; the marker workgroup is k_sweep_lists' -- its points and its count are plain stores already. */
__global__ __launch_bounds__(384) void k_sweep_lists_direct(urf_kargs a, urf_dev_params dp, urf_sweep_lists_args o)
{
    if (blockIdx.x < (unsigned)dp.p.channels) {   /* (uniform) */
        urf_ordered_lists<384, true>(a, dp, 0u, o.rord, o.rcls, o.road, nullptr, nullptr, 0u, o.list_counts);
        return;
    }
    urf_sweep_marker_bins(a, o);
}

#ifdef URF_ENABLE_TEST_HOOKS   /* liburf_hip_test.so only (include/urf_test_hooks.h) */
/* ------------------------------------------------------------------------- */
/* self test                                                                   */
/* ------------------------------------------------------------------------- */
/* urf_div_pi(a) == a / M_PI for every float a in [0, 600] (bit patterns 0..0x44160000) */
__global__ __launch_bounds__(256) void k_selftest_div_pi(unsigned long long* mismatches)
{
    const unsigned top = 0x44160000u;   /* 600.0f */
    unsigned long long bad = 0;
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b <= top;
         b += (unsigned long long)gridDim.x * blockDim.x) {
        const double a = (double)__uint_as_float((unsigned)b);
        if (urf_div_pi(a) != a / URF_PI_D)
            bad++;
    }
    /* urf_sqrt_rn_normal(x) == sqrtf(x) for every float of [2^-90, 2^126] (k_front's planar range) */
    for (unsigned long long b = 0x12800000ull + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b <= 0x7e800000ull;
         b += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((unsigned)b);
        if (__float_as_uint(urf_sqrt_rn_normal(x)) != __float_as_uint(__builtin_sqrtf(x)))
            bad++;
    }
    if (bad)
        atomicAdd(mismatches, bad);
}

/* max |fast - exact| of the float fast paths over pseudo-random points: out[0] = vertical angle
 * [deg] (float bits), out[1] = polar angle [rad], out[2] = scaled polar angle fi*Kfi, out[3] =
 * azimuth [deg] */
__global__ __launch_bounds__(256) void k_selftest_fast(unsigned long long n, float Kfi, unsigned* out)
{
    float ev = 0.f, ea = 0.f, eu = 0.f, ez = 0.f;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned long long h = i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        float c[3];
        for (int k = 0; k < 3; k++) {
            h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27; h *= 0x94D049BB133111EBull; h ^= h >> 31;
            c[k] = ((float)(h >> 40) * (1.0f / 16777216.0f) - 0.5f) * ((i & 3) == 0 ? 400.0f : 20.0f);
        }
        /* an eighth of the samples at arbitrary magnitudes (2^-70 .. 2^70), with independent
         * exponents per coordinate: the range guards of the fast paths have to hold there too */
        if ((i & 7) == 1) {
            for (int k = 0; k < 3; k++) {
                h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27;
                c[k] = __builtin_ldexpf(c[k], (int)(h % 141u) - 70);
            }
        }
        /* another eighth close to the x axis (|y| / |x| between 1 / 2048 and 1 / 8), where the azimuth's
         * margin grows with 1 / delta and its end (urf_fast_az_ok) lies */
        if ((i & 7) == 2) {
            h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 27;
            c[1] = c[0] * __builtin_ldexpf(1.0f + (float)(h >> 41) * (1.0f / 8388608.0f), -(int)(4 + (h & 7u))) * ((h & 8u) ? -1.0f : 1.0f);
        }
        const float x = c[0], y = c[1], z = c[2] * 0.25f;
        float vt;
        if (urf_fast_vertical_angle(x, y, z, &vt)) {   /* k_ring_table's look-ahead */
            const float d = __builtin_fabsf(vt - urf_vertical_angle(x, y, z));
            ev = d > ev ? d : ev;
        }
        float uc;
        bool planar_ok;
        if (urf_fast_cot(x, y, z, &uc, &planar_ok)) {   /* k_split: the angle whose cotangent uc is (atan2 rounded to float: +-1e-5 deg) */
            const float au = (float)((double)urf_atan2f(1.0f, uc) * (180.0 / URF_PI_D));
            const float d = __builtin_fabsf(au - urf_vertical_angle(x, y, z));
            ev = d > ev ? d : ev;
        }
        float azt;
        if (urf_fast_azimuth(x, y, &azt)) {
            float d2;
            const float d = __builtin_fabsf(azt - urf_azimuth(x, y, &d2)) / urf_fast_az_eps(azt);   /* as a fraction of the margin */
            if (d < 1000.0f)   /* the 0/360 seam is never decided on the approximation */
                ez = d > ez ? d : ez;
        }
        if (x != 0.f || y != 0.f) {
            float fe = urf_atan2f(y, x);
            const float fa = urf_fast_atan2f(y, x);
            const float da = __builtin_fabsf(fa - fe);
            ea = da > ea ? da : ea;
            if (fe < 0.0f)
                fe = (float)((double)fe + 2.0 * URF_PI_D);
            float ff = fa < 0.0f ? fa + 6.28318530717958648f : fa;
            /* near the wrap the two may sit on opposite ends: the fast path never decides there */
            const float du = __builtin_fabsf(ff * Kfi - fe * Kfi);
            if (du < 180.0f)
                eu = du > eu ? du : eu;
        }
    }
    atomicMax(&out[0], __float_as_uint(ev));
    atomicMax(&out[1], __float_as_uint(ea));
    atomicMax(&out[2], __float_as_uint(eu));
    atomicMax(&out[3], __float_as_uint(ez));
}
#endif   /* URF_ENABLE_TEST_HOOKS */


#endif /* URF_K_OUTPUTS_HPP */
