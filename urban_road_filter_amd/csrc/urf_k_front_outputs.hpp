/*
 * urf_k_front_outputs.hpp -- the published order and the road_marker points of a scan that took the fused front end (urf_front.hpp: any
 * laser count), straight from what that call left on the device (urf_set_front_outputs): siblings of urf_k_outputs.hpp's
 * k_ring_order, k_marker_ring, k_marker_ring_literal and k_marker_bins under their own names.
 *
 * A fused scan keeps no ring-sorted copies.  Its ring r is one laser slot, its j-th point the j-th set bit of that slot's presence
 * words (front_pres / front_pres128: word (f >> 5) * L + l, bit f & 31) in firing order -- the order the reference's bucketing
 * leaves before its quicksort (lidar_segmentation.cpp:226-242, 289-291) --, k_front_finish has written ring_cnt.
 *
 *   k_front_out_prep   grid (tiles, scans) x 256 threads, the tile pre-pass, ONCE per recorded call (the host keeps a mark): reads a tile's
 *                      x / y in firing order (the caller's arrays, or k_transpose's copy of a row-major sweep: urf_front_src) and its
 *                      labels, coalesced as k_front does, ranks every present point inside its laser slot with popcounts over the
 *                      presence words, and leaves per ring-major position rel + j (rel: exclusive scan of ring_cnt, worked out here --
 *                      the fused path does not fill ring_off; the scan's first block stores the row for k_ordered_lists) the bits of
 *                      the exact azimuth, the entry input index | class << 30 and the planar distance.  A slot's points of one tile are
 *                      consecutive positions: the tile's values are staged in LDS slot by slot and leave as one stretch per slot (a
 *                      wave's store straight from the march order would touch 64 cache lines with four bytes each).  Nobody writes
 *                      these arrays afterwards -- the sorts work in LDS or in the ring's stretch of wsg --, so one pre-pass serves
 *                      the published order and the marker tables.  The per-ring kernels read contiguous memory.
 *   k_ring_order_front, k_marker_ring_front, k_marker_ring_literal_front, k_marker_bins_front
 *                      launched on the grids of their general counterparts, which return at once for a fused scan (urf_scan_fused) as
 *                      these do for every other.  They hold no rule of their own: ties, the literal quicksort, (d, first in ring order)
 *                      live once in urf_k_readouts.hpp, templated on a ring view, and a kernel here is its launch shape, its early
 *                      returns and the view urf_ring_fused over the pre-pass's arrays.  (The one place that states those rules a second
 *                      time is on the other side: k_marker_ring's register-resident path for rings of up to 2048 points.)
 *
 * Precondition: k_front hands back every scan with a ring point on the sensor's axis, so a fused scan has no NaN azimuth
 * (urf_ring_fused::MAY_NAN).
 */
#ifndef URF_K_FRONT_OUTPUTS_HPP
#define URF_K_FRONT_OUTPUTS_HPP

/* out[i] = in[0] + .. + in[i - 1] for i = 0 .. n (n <= 128), by the workgroup's first wave: two elements per lane */
__device__ __forceinline__ void urf_fout_excl_scan(const unsigned* in, unsigned* out, unsigned n, unsigned tid)
{
    if (tid < 64u) {   /* (uniform per wave) */
        const unsigned i0 = 2u * tid, i1 = i0 + 1u;
        const unsigned v0 = i0 < n ? in[i0] : 0u, v1 = i1 < n ? in[i1] : 0u;
        const unsigned inc = urf_wave_scan_add(v0 + v1);
        if (i0 <= n)
            out[i0] = inc - v0 - v1;
        if (i1 <= n)
            out[i1] = inc - v1;
        if (tid == 63u && n == 128u)
            out[128] = inc;
    }
}

__global__ __launch_bounds__(256) void k_front_out_prep(urf_kargs a, urf_dev_params dp, unsigned s0, unsigned* az_all, unsigned* ent_all,
                                                        float* d_all)
{
    constexpr unsigned EPT = URF_TILE / 256u, NONE = 0xffffffffu;
    __shared__ unsigned lane_base[128], lane_rel[128], lane_cnt[128], lane_off[129], roff[URF_MAX_CHANNELS + 1], rcnt[URF_MAX_CHANNELS];
    __shared__ unsigned st_az[URF_TILE], st_ent[URF_TILE];
    __shared__ float st_d[URF_TILE];
    const unsigned t = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    const urf_scan_info in = a.info[s];
    if (!urf_scan_fused(a, s, in))
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    if (t * URF_TILE >= len)
        return;
    const unsigned lsh = a.front_lsh, L = 1u << lsh, lm = L - 1u;
    const unsigned C = (unsigned)dp.p.channels;
    const bool rows = a.front_ok[s] == URF_FRONT_ROWS;   /* (uniform) labels and input indices are row-major: l * F + f */
    const unsigned F = len >> lsh;
    const uint32_t* const pres = urf_front_pres_of(a, s);   /* (urf_front_lay, urf_front.hpp: either family's) */
    const uint32_t* const lane_ring = urf_front_lane_ring_of(a, s);
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, a.front_ok[s], gx, gy, gz);
    const size_t ob = (size_t)blockIdx.y * a.sstride;
    if (tid < 128) {
        lane_base[tid] = 0;
        lane_cnt[tid] = 0;
    }
    if (tid < URF_MAX_CHANNELS)
        rcnt[tid] = tid < C ? a.ring_cnt[(size_t)s * C + tid] : 0u;
    __syncthreads();
    urf_fout_excl_scan(rcnt, roff, C, tid);   /* ring points of the scan in front of every ring */
    /* the slot's ring points in front of the tile: whole presence words, then (128 lasers: a word covers two tiles) the bits of the tile's
     * first word that belong to the tile before */
    const unsigned f0 = (t * URF_TILE) >> lsh, w0 = f0 >> 5;
    const unsigned m0 = ~((1u << (f0 & 31u)) - 1u);   /* bits of word w0 from the tile's first firing on */
    {
        const unsigned l = tid & lm, part = tid >> lsh, parts = 256u >> lsh;
        unsigned run = 0;
        for (unsigned w = part; w < w0; w += parts)
            run += (unsigned)__popc(pres[(size_t)w * L + l]);
        if (run)
            atomicAdd(&lane_base[l], run);
    }
    __syncthreads();
    if (t == 0 && tid <= C)
        a.ring_off[(size_t)s * (C + 1) + tid] = roff[tid];   /* k_ordered_lists and the siblings read the row */
    if (tid < L) {
        const unsigned r = lane_ring[tid];
        lane_rel[tid] = r < C ? roff[r] : NONE;   /* (a slot that met no ring holds no ring point) */
        lane_base[tid] += (unsigned)__popc(pres[(size_t)w0 * L + tid] & ~m0);
    }
    __syncthreads();
    /* pass 1: the thread's eight points -- values in registers, place = (slot, rank among the slot's points of this tile) */
    unsigned vaz[EPT], vent[EPT], vloc[EPT];
    float vd[EPT];
#pragma unroll
    for (unsigned q = 0; q < EPT; q++) {
        const unsigned i = t * URF_TILE + q * 256u + tid;
        vloc[q] = NONE;
        vaz[q] = vent[q] = 0u;
        vd[q] = 0.f;
        if (i < len) {
            const unsigned f = i >> lsh, l = i & lm, w = f >> 5;
            const unsigned word = pres[(size_t)w * L + l];
            if (((word >> (f & 31u)) & 1u) && lane_rel[l] != NONE) {
                unsigned jl = (unsigned)__popc(word & ((1u << (f & 31u)) - 1u) & (w == w0 ? m0 : 0xffffffffu));
                for (unsigned v = w0; v < w; v++)   /* (16 / 32 lasers: a tile spans four / two words) */
                    jl += (unsigned)__popc(pres[(size_t)v * L + l] & (v == w0 ? m0 : 0xffffffffu));
                const unsigned src = rows ? l * F + f : i;
                const unsigned cls = a.labels[(size_t)off + src] & URF_LABEL_MASK;
                float d;
                vaz[q] = urf_fbits(urf_azimuth(gx[i], gy[i], &d));
                vd[q] = d;
                vent[q] = src | (cls << 30);
                vloc[q] = (l << 16) | jl;
                atomicAdd(&lane_cnt[l], 1u);
            }
        }
    }
    __syncthreads();
    urf_fout_excl_scan(lane_cnt, lane_off, L, tid);
    __syncthreads();
    /* pass 2: slot by slot into LDS */
#pragma unroll
    for (unsigned q = 0; q < EPT; q++)
        if (vloc[q] != NONE) {
            const unsigned k = lane_off[vloc[q] >> 16] + (vloc[q] & 0xffffu);
            st_az[k] = vaz[q];
            st_ent[k] = vent[q];
            st_d[k] = vd[q];
        }
    __syncthreads();
    /* pass 3: every slot's stretch to its ring-major positions */
    const unsigned total = lane_off[L];
    for (unsigned k = tid; k < total; k += 256u) {
        unsigned lo = 0, hi = L;   /* the largest slot with lane_off <= k (it is not empty: lane_off of the next one lies above k) */
        while (hi - lo > 1u) {
            const unsigned mid = (lo + hi) >> 1;
            if (lane_off[mid] <= k)
                lo = mid;
            else
                hi = mid;
        }
        const size_t p = ob + lane_rel[lo] + lane_base[lo] + (k - lane_off[lo]);
        az_all[p] = st_az[k];
        ent_all[p] = st_ent[k];
        d_all[p] = st_d[k];
    }
}

/* The ring of a fused scan as the shared bodies reach it (urf_ring_fused): its stretch of k_front_out_prep's arrays.  d_all: where distances
 * are read (the marker kernels). */
__device__ __forceinline__ urf_ring_fused urf_fout_ring(const urf_kargs& a, unsigned s, unsigned C, unsigned c, unsigned scan_of_launch,
                                                        const unsigned* az_all, const unsigned* ent_all, const float* d_all)
{
    const size_t ro = (size_t)scan_of_launch * a.sstride + a.ring_off[(size_t)s * (C + 1) + c];
    return urf_ring_fused{ az_all + ro, ent_all + ro, d_all ? d_all + ro : nullptr };
}

/* k_ring_order for a fused scan: the key of position i is (az[i], i).  Rings beyond 2048 points are sorted in the ring's stretch of wsg, which
 * is the array of the literal pass as well. */
__global__ __launch_bounds__(256) void k_ring_order_front(urf_kargs a, urf_dev_params dp, unsigned s0, const unsigned* az_all,
                                                          const unsigned* ent_all, unsigned* rord_all, unsigned* rcls_all)
{
    constexpr unsigned NT = 256, NB = 2048, EPT = 8, CAP = NT * EPT;
    __shared__ unsigned long long A[CAP];
    __shared__ unsigned cnt[URF_BLOCK_CNT(NB, NT)];
    __shared__ urf_sort_shared ssh;
    __shared__ unsigned ncls[2], sh_tie;
    __shared__ int lom_stk[2 * 64];
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    const urf_scan_info in = a.info[s];
    if (!urf_scan_fused(a, s, in))
        return;
    unsigned* rcls = rcls_all + ((size_t)blockIdx.y * URF_MAX_CHANNELS + c) * 2;
    if (c >= in.n_rings) {
        if (tid < 2)
            rcls[tid] = 0;
        return;
    }
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    unsigned* const rord = rord_all + (size_t)blockIdx.y * a.sstride + rel;
    const urf_ring_fused v = urf_fout_ring(a, s, C, c, blockIdx.y, az_all, ent_all, nullptr);
    if (tid < 2)
        ncls[tid] = 0;
    if (tid == 0)
        sh_tie = 0;
    __syncthreads();
    unsigned long long* const G = (unsigned long long*)(a.wsg + urf_sbase(a, s) + rel);
    volatile unsigned long long* const LIT = G;
    unsigned my_road = 0, my_curb = 0;
    if (n <= CAP) {
        unsigned long long key[EPT];
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {
            const unsigned i = tid + e * NT;
            key[e] = i < n ? urf_ring_key(v, i) : ~0ull;
        }
        urf_block_sort_keys<NT, EPT, NB>(key, n, A, cnt, &ssh, false);
        const bool lit = urf_ring_literal_order<NT>(v, n, A, LIT, &sh_tie, lom_stk, tid);
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {
            const unsigned j = tid + e * NT;
            if (j < n)
                urf_ring_publish(v, lit ? (unsigned)LIT[j] : (unsigned)A[j], &rord[j], my_road, my_curb);
        }
    } else
        urf_ring_order_long<NT>(v, n, G, LIT, &sh_tie, lom_stk, rord, my_road, my_curb, tid);
    urf_ring_publish_counts(my_road, my_curb, ncls, rcls, tid);
}

/* k_marker_ring for a fused scan: every ring pass by pass (its points lie contiguous: nothing to keep in registers).  m_pos holds the marker
 * point's input index, relative to the scan (urf_ring_fused::marker_id). */
__global__ __launch_bounds__(256) void k_marker_ring_front(urf_kargs a, urf_dev_params dp, unsigned s0, const unsigned* az_all,
                                                           const unsigned* ent_all, const float* d_all, float* m_d_all, unsigned* m_pos_all,
                                                           uint8_t* m_red_all, uint8_t* m_lit_all)
{
    __shared__ urf_marker_tabs T;
    __shared__ unsigned need_lit;
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    const urf_scan_info in = a.info[s];
    if (!urf_scan_fused(a, s, in))
        return;
    if (c >= in.n_rings) {
        if (tid == 0)
            m_lit_all[(size_t)blockIdx.y * URF_MAX_CHANNELS + c] = 0;
        return;
    }
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    const unsigned C = (unsigned)dp.p.channels;
    const urf_ring_fused v = urf_fout_ring(a, s, C, c, blockIdx.y, az_all, ent_all, d_all);
    T.init(tid);
    if (tid == 0)
        need_lit = 0;
    __syncthreads();
    urf_marker_passes(v, a.ring_cnt[(size_t)s * C + c], T, &need_lit, tid);
    if (tid == 0)
        m_lit_all[(size_t)blockIdx.y * URF_MAX_CHANNELS + c] = (uint8_t)need_lit;
    T.store(v, c, m_d_all + blockIdx.y * cells, m_pos_all + blockIdx.y * cells, m_red_all + blockIdx.y * cells, tid);
}

/* k_marker_ring_literal for a fused scan: the rings k_marker_ring_front flagged, sorted literally in the ring's stretch of wsg. */
__global__ __launch_bounds__(256) void k_marker_ring_literal_front(urf_kargs a, urf_dev_params dp, unsigned s0, const uint8_t* m_lit_all,
                                                                   const unsigned* az_all, const unsigned* ent_all,
                                                                   const float* d_all, float* m_d_all, unsigned* m_pos_all, uint8_t* m_red_all)
{
    const unsigned c = blockIdx.x, s = s0 + blockIdx.y, tid = threadIdx.x;
    const urf_scan_info in = a.info[s];
    if (!urf_scan_fused(a, s, in) || !m_lit_all[(size_t)blockIdx.y * URF_MAX_CHANNELS + c])
        return;
    __shared__ urf_marker_tabs T;
    __shared__ int stk[2 * 64];
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    const unsigned C = (unsigned)dp.p.channels;
    const urf_ring_fused v = urf_fout_ring(a, s, C, c, blockIdx.y, az_all, ent_all, d_all);
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    urf_marker_literal(v, a.ring_cnt[(size_t)s * C + c], (volatile unsigned long long*)(a.wsg + urf_sbase(a, s) + rel), T, stk, tid);
    T.store(v, c, m_d_all + blockIdx.y * cells, m_pos_all + blockIdx.y * cells, m_red_all + blockIdx.y * cells, tid);
}

/* k_marker_bins for a fused scan: m_pos holds input indices, the point comes from the call's input arrays. */
__global__ __launch_bounds__(384) void k_marker_bins_front(urf_kargs a, urf_dev_params dp, unsigned s0, const float* m_d_all,
                                                           const unsigned* m_pos_all, const uint8_t* m_red_all, float* out_all,
                                                           unsigned* count_all)
{
    __shared__ unsigned wsum[6];
    const unsigned s = s0 + blockIdx.x;
    const urf_scan_info in = a.info[s];
    if (!urf_scan_fused(a, s, in))
        return;
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    urf_marker_bins<urf_ring_fused>(a, off, in.n_rings, m_d_all + blockIdx.x * cells, m_pos_all + blockIdx.x * cells,
                                    m_red_all + blockIdx.x * cells, out_all + (size_t)blockIdx.x * URF_DEG_CELLS * 4, count_all + blockIdx.x, wsum);
}

#endif /* URF_K_FRONT_OUTPUTS_HPP */
