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
 *                      these do for every other; the rules -- ties, the literal quicksort, (d, first in ring order) -- are theirs,
 *                      word for word.
 *
 * Precondition: k_front hands back every scan with a ring point on the sensor's axis, so a fused scan has no NaN azimuth.
 */
#ifndef URF_K_FRONT_OUTPUTS_HPP
#define URF_K_FRONT_OUTPUTS_HPP

#define URF_FOUT_SRC_MASK 0x3fffffffu   /* entry = input index (relative to the scan) | class << 30 */

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

/* k_ring_order for a fused scan: the azimuth bits of the ring's points lie contiguous in az_all (k_front_out_prep), the key of position i
 * is (bits, i).  Rings beyond 2048 points are sorted in the ring's stretch of wsg. */
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
    unsigned* rord = rord_all + (size_t)blockIdx.y * a.sstride;
    unsigned* rcls = rcls_all + ((size_t)blockIdx.y * URF_MAX_CHANNELS + c) * 2;
    if (c >= in.n_rings) {
        if (tid < 2)
            rcls[tid] = 0;
        return;
    }
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    const unsigned sb = urf_sbase(a, s);
    const unsigned* const az = az_all + (size_t)blockIdx.y * a.sstride + rel;
    const unsigned* const ent = ent_all + (size_t)blockIdx.y * a.sstride + rel;
    auto key_of = [&](unsigned i) { return ((unsigned long long)az[i] << 32) | i; };
    if (tid < 2)
        ncls[tid] = 0;
    if (tid == 0)
        sh_tie = 0;
    __syncthreads();
    /* equal azimuths: k_ring_order's literal_order (the keys in bucket order are the keys by position; SORTED may be LIT itself: it is
     * read before the barrier and written behind it) */
    volatile unsigned long long* const LIT = (volatile unsigned long long*)(a.wsg + sb + rel);
    auto literal_order = [&](const unsigned long long* SORTED) -> bool {
        for (unsigned j = tid; j + 1 < n; j += NT)
            if ((unsigned)(SORTED[j] >> 32) == (unsigned)(SORTED[j + 1] >> 32))
                sh_tie = 1u;
        __syncthreads();
        if (!sh_tie)
            return false;   /* (uniform) */
        for (unsigned j = tid; j < n; j += NT)
            LIT[j] = key_of(j);
        __threadfence_block();
        __syncthreads();
        if (tid < 64)
            urf_lomuto_sort(LIT, n, lom_stk);
        __threadfence_block();
        __syncthreads();
        return true;
    };
    unsigned my_road = 0, my_curb = 0;
    auto publish = [&](unsigned j, unsigned pos) {
        const unsigned e = ent[pos], cls = e >> 30;
        rord[rel + j] = e;
        my_road += cls == URF_LABEL_ROAD;
        my_curb += cls == URF_LABEL_CURB;
    };
    if (n <= CAP) {
        unsigned long long key[EPT];
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {
            const unsigned i = tid + e * NT;
            key[e] = i < n ? key_of(i) : ~0ull;
        }
        urf_block_sort_keys<NT, EPT, NB>(key, n, A, cnt, &ssh, false);
        const bool lit = literal_order(A);
#pragma unroll
        for (unsigned e = 0; e < EPT; e++) {
            const unsigned j = tid + e * NT;
            if (j < n)
                publish(j, lit ? (unsigned)LIT[j] : (unsigned)A[j]);
        }
    } else {
        unsigned long long* const G = (unsigned long long*)(a.wsg + sb + rel);
        for (unsigned i = tid; i < n; i += NT)
            G[i] = key_of(i);
        __threadfence_block();
        __syncthreads();
        unsigned P = 1;
        while (P < n)
            P <<= 1;
        for (unsigned kk = 2; kk <= P; kk <<= 1)
            for (unsigned j = kk >> 1; j > 0; j >>= 1) {
                const bool flip = (j == (kk >> 1));
                for (unsigned tt = tid; tt < (P >> 1); tt += NT) {
                    const unsigned lo = ((tt & ~(j - 1)) << 1) | (tt & (j - 1));
                    const unsigned hi = flip ? ((lo & ~(kk - 1)) + (kk - 1) - (lo & (kk - 1))) : lo + j;
                    if (hi < n) {
                        const unsigned long long ka = G[lo], kb = G[hi];
                        if (ka > kb) {
                            G[lo] = kb;
                            G[hi] = ka;
                        }
                    }
                }
                __threadfence_block();
                __syncthreads();
            }
        const bool lit = literal_order(G);
        for (unsigned j = tid; j < n; j += NT)
            publish(j, lit ? (unsigned)LIT[j] : (unsigned)G[j]);
    }
    if (my_road)
        atomicAdd(&ncls[0], my_road);
    if (my_curb)
        atomicAdd(&ncls[1], my_curb);
    __syncthreads();
    if (tid < 2)
        rcls[tid] = ncls[tid];
}

/* k_marker_ring for a fused scan: azimuth bits, class and planar distance of the ring's points lie contiguous (k_front_out_prep,
 * azimuth bits by position).  m_pos holds the marker point's input index, relative to the scan (k_marker_bins_front). */
__global__ __launch_bounds__(256) void k_marker_ring_front(urf_kargs a, urf_dev_params dp, unsigned s0, const unsigned* az_all,
                                                           const unsigned* ent_all, const float* d_all, float* m_d_all, unsigned* m_pos_all,
                                                           uint8_t* m_red_all, uint8_t* m_lit_all)
{
    __shared__ int nrmin[URF_DEG_CELLS];
    __shared__ unsigned long long best[URF_DEG_CELLS];
    __shared__ unsigned bestpos[URF_DEG_CELLS];
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
    float* m_d = m_d_all + blockIdx.y * cells;
    unsigned* m_pos = m_pos_all + blockIdx.y * cells;
    uint8_t* m_red = m_red_all + blockIdx.y * cells;
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const size_t ro = (size_t)blockIdx.y * a.sstride + a.ring_off[(size_t)s * (C + 1) + c];
    const unsigned* const az = az_all + ro;
    const unsigned* const ent = ent_all + ro;
    const float* const dist = d_all + ro;
    for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
        nrmin[i] = URF_INT_NONE_MIN;
        best[i] = 0;
        bestpos[i] = 0xffffffffu;
    }
    if (tid == 0)
        need_lit = 0;
    __syncthreads();
    auto bin_of = [](float az) {
        const int b = (int)__builtin_floorf(az);
        return b < 0 ? 0 : (b > 360 ? 360 : b);
    };
    /* pass 1: where does the scan of this ring stop in each degree (:318) */
    for (unsigned p = tid; p < n; p += 256) {
        const unsigned ab = az[p];
        if ((ent[p] >> 30) != URF_LABEL_ROAD)
            atomicMin(&nrmin[bin_of(__uint_as_float(ab))], (int)ab);
    }
    __syncthreads();
    /* pass 2: farthest road point in front of it (:325-335); key = (d, first in azimuth order) */
    for (int pass = 0; pass < 2; pass++) {
        for (unsigned p = tid; p < n; p += 256) {
            const unsigned ab = az[p];
            if ((ent[p] >> 30) != URF_LABEL_ROAD)
                continue;
            const int bin = bin_of(__uint_as_float(ab));
            if ((int)ab == nrmin[bin])
                need_lit = 1u;   /* the very azimuth of the degree's first non-road point: in front of it or behind? */
            if ((int)ab < nrmin[bin]) {
                const float d = dist[p];
                if (d > 0.0f) {   /* "d > maxDistanceRoad" with maxDistanceRoad starting at 0 */
                    const unsigned long long k = ((unsigned long long)urf_fbits(d) << 32) | (0xffffffffu - ab);
                    if (pass == 0)
                        atomicMax(&best[bin], k);
                    else if (k == best[bin] && atomicMin(&bestpos[bin], p) != 0xffffffffu)
                        need_lit = 1u;   /* two road points with this distance AND azimuth: which comes first? */
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0)
        m_lit_all[(size_t)blockIdx.y * URF_MAX_CHANNELS + c] = (uint8_t)need_lit;
    for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
        const size_t o = (size_t)c * URF_DEG_CELLS + i;
        m_d[o] = __uint_as_float((unsigned)(best[i] >> 32));
        m_pos[o] = bestpos[i] == 0xffffffffu ? 0xffffffffu : ent[bestpos[i]] & URF_FOUT_SRC_MASK;
        m_red[o] = nrmin[i] != URF_INT_NONE_MIN;
    }
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
    __shared__ int nrmin[URF_DEG_CELLS];
    __shared__ unsigned long long best[URF_DEG_CELLS];
    __shared__ unsigned bestpos[URF_DEG_CELLS];
    __shared__ int stk[2 * 64];
    const size_t cells = (size_t)URF_MAX_CHANNELS * URF_DEG_CELLS;
    float* m_d = m_d_all + blockIdx.y * cells;
    unsigned* m_pos = m_pos_all + blockIdx.y * cells;
    uint8_t* m_red = m_red_all + blockIdx.y * cells;
    const unsigned C = (unsigned)dp.p.channels;
    const unsigned n = a.ring_cnt[(size_t)s * C + c];
    const unsigned rel = a.ring_off[(size_t)s * (C + 1) + c];
    const size_t ro = (size_t)blockIdx.y * a.sstride + rel;
    const unsigned* const az = az_all + ro;
    const unsigned* const ent = ent_all + ro;
    const float* const dist = d_all + ro;
    volatile unsigned long long* const LIT = (volatile unsigned long long*)(a.wsg + urf_sbase(a, s) + rel);
    for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
        nrmin[i] = URF_INT_NONE_MIN;
        best[i] = 0;
        bestpos[i] = 0xffffffffu;
    }
    for (unsigned p = tid; p < n; p += 256)
        LIT[p] = ((unsigned long long)az[p] << 32) | p;   /* (azimuth bits, position), in ring order */
    __threadfence_block();
    __syncthreads();
    if (tid < 64 && n >= 2)
        urf_lomuto_sort(LIT, n, stk);
    __threadfence_block();
    __syncthreads();
    for (int pass = 0; pass < 3; pass++) {
        for (unsigned j = tid; j < n; j += 256) {
            const unsigned long long e = LIT[j];
            const float az = urf_pair_alpha(e);
            const unsigned p = (unsigned)e;
            const unsigned lab = ent[p] >> 30;
            int bin = (int)__builtin_floorf(az);
            bin = bin < 0 ? 0 : (bin > 360 ? 360 : bin);
            if (pass == 0) {
                if (lab != URF_LABEL_ROAD)
                    atomicMin(&nrmin[bin], (int)j);   /* :318 the scan of this ring stops here */
            } else if (lab == URF_LABEL_ROAD && (int)j < nrmin[bin]) {
                const float d = dist[p];
                if (d > 0.0f) {
                    const unsigned long long k = ((unsigned long long)urf_fbits(d) << 32) | (0xffffffffu - j);   /* (d, first in the ring's order) */
                    if (pass == 1)
                        atomicMax(&best[bin], k);
                    else if (k == best[bin])
                        bestpos[bin] = p;
                }
            }
        }
        __syncthreads();
    }
    for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
        const size_t o = (size_t)c * URF_DEG_CELLS + i;
        m_d[o] = __uint_as_float((unsigned)(best[i] >> 32));
        m_pos[o] = bestpos[i] == 0xffffffffu ? 0xffffffffu : ent[bestpos[i]] & URF_FOUT_SRC_MASK;
        m_red[o] = nrmin[i] != URF_INT_NONE_MIN;
    }
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
    const float* m_d = m_d_all + blockIdx.x * cells;
    const unsigned* m_pos = m_pos_all + blockIdx.x * cells;
    const uint8_t* m_red = m_red_all + blockIdx.x * cells;
    float* out = out_all + (size_t)blockIdx.x * URF_DEG_CELLS * 4;
    unsigned* count = count_all + blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned nR = in.n_rings;
    unsigned id = 0xffffffffu;
    float red = 0.f;
    if (tid <= 360) {
        float maxd = 0.f;
        for (unsigned j = 0; j < nR; j++) {
            const size_t o = (size_t)j * URF_DEG_CELLS + tid;
            if (m_pos[o] != 0xffffffffu && m_d[o] > maxd) {   /* :329 */
                maxd = m_d[o];
                id = m_pos[o];
            }
            if (m_red[o]) {                                  /* :318-321, 338-339 */
                red = 1.f;
                break;
            }
        }
    }
    const bool valid = id != 0xffffffffu;                    /* :343 */
    const unsigned long long m = __ballot(valid);
    if (lane == 0)
        wsum[wave] = __popcll(m);
    __syncthreads();
    unsigned pre = __popcll(m & ((1ull << lane) - 1ull));
    for (unsigned w = 0; w < wave; w++)
        pre += wsum[w];
    if (valid) {
        out[4 * pre + 0] = a.x[(size_t)off + id];
        out[4 * pre + 1] = a.y[(size_t)off + id];
        out[4 * pre + 2] = a.z[(size_t)off + id];
        out[4 * pre + 3] = red;
    }
    if (tid == 0)
        *count = wsum[0] + wsum[1] + wsum[2] + wsum[3] + wsum[4] + wsum[5];
}

#endif /* URF_K_FRONT_OUTPUTS_HPP */
