/*
 * urf_k_readouts.hpp -- the rules of the published order and of the road_marker tables, once, for the kernels of urf_k_outputs.hpp (scans
 * with ring-sorted copies) and of urf_k_front_outputs.hpp (scans of the fused front end).  The two kinds of scan differ in how a ring's
 * points are reached -- the ring view -- and in nothing else: ties between bit-equal azimuths, the literal quicksort, (d, first in ring
 * order) live in the bodies below, templated on the view.
 *
 * A ring view is built per (scan, ring).  at(i) turns position i of the ring (bucket order: what the reference's quicksort starts from)
 * into a handle, the other members read one property of the point behind a handle:
 *   az_bits      bits of the exact azimuth
 *   entry        what is published: input index (relative to the scan) | class << 30, and the class
 *   cls          the class alone
 *   dist         planar distance as the reference rounds it (each view keeps its own source: both match the reference bit for bit)
 *   marker_id    what the marker tables keep for the point; marker_point (static: k_marker_bins has no ring) resolves it to x, y, z
 *   MAY_NAN      whether an azimuth may be NaN; where it may not, the tests fold away
 */
#ifndef URF_K_READOUTS_HPP
#define URF_K_READOUTS_HPP

#define URF_FOUT_SRC_MASK 0x3fffffffu   /* entry = input index (relative to the scan) | class << 30 */

/* Ring c of a scan with ring-sorted copies; handle = ring-sorted slot, relative to the scan's scratch base sb.  map: the ring's run table
 * in LDS where the kernel keeps one (k_ring's map), else nullptr: the bisection in global memory (urf_ring_slot). */
struct urf_ring_sorted {
    static constexpr bool MAY_NAN = true;   /* a ring point on the sensor's axis */
    const urf_kargs& a;
    unsigned s, C, c, ntiles, sb, off;
    const urf_ring_map* map;
    __device__ __forceinline__ unsigned at(unsigned i) const { return map ? map->at(i) : urf_ring_slot(a, s, C, c, ntiles, i); }
    __device__ __forceinline__ unsigned az_bits(unsigned slot) const { return urf_fbits(urf_exact_az(a, sb + slot)); }
    __device__ __forceinline__ unsigned entry(unsigned slot, unsigned& cls) const
    {
        const unsigned src = (slot & ~(URF_TILE - 1u)) + (a.rec[sb + slot] & URF_REC_SRC_MASK);
        cls = a.labels[off + src] & URF_LABEL_MASK;
        return src | (cls << 30);
    }
    __device__ __forceinline__ unsigned cls(unsigned slot) const
    {
        unsigned k;
        entry(slot, k);
        return k;
    }
    __device__ __forceinline__ float dist(unsigned slot) const
    {
        const float x = a.rx[sb + slot], y = a.ry[sb + slot];
        return (float)__builtin_sqrt((double)(0.f - x) * (double)(0.f - x) + (double)(0.f - y) * (double)(0.f - y));
    }
    __device__ __forceinline__ unsigned marker_id(unsigned slot) const { return sb + slot; }   /* absolute scratch slot */
    static __device__ __forceinline__ void marker_point(const urf_kargs& a, unsigned, unsigned id, float* o)
    {
        o[0] = a.rx[id];
        o[1] = a.ry[id];
        o[2] = a.rz[id];
    }
};

/* A ring of a fused scan; handle = the position itself: azimuth bits, entry and planar distance lie contiguous by ring position
 * (k_front_out_prep).  k_front hands back every scan with a ring point on the sensor's axis: no NaN azimuth. */
struct urf_ring_fused {
    static constexpr bool MAY_NAN = false;
    const unsigned *az, *ent;
    const float* d;
    __device__ __forceinline__ unsigned at(unsigned i) const { return i; }
    __device__ __forceinline__ unsigned az_bits(unsigned i) const { return az[i]; }
    __device__ __forceinline__ unsigned entry(unsigned i, unsigned& cls) const
    {
        const unsigned e = ent[i];
        cls = e >> 30;
        return e;
    }
    __device__ __forceinline__ unsigned cls(unsigned i) const { return ent[i] >> 30; }
    __device__ __forceinline__ float dist(unsigned i) const { return d[i]; }
    __device__ __forceinline__ unsigned marker_id(unsigned i) const { return ent[i] & URF_FOUT_SRC_MASK; }   /* input index, relative to the scan */
    static __device__ __forceinline__ void marker_point(const urf_kargs& a, unsigned off, unsigned id, float* o)
    {
        o[0] = a.x[(size_t)off + id];
        o[1] = a.y[(size_t)off + id];
        o[2] = a.z[(size_t)off + id];
    }
};

template <class V>
__device__ __forceinline__ unsigned long long urf_ring_key(const V& v, unsigned i)   /* (azimuth bits, position in the ring) */
{
    return ((unsigned long long)v.az_bits(v.at(i)) << 32) | i;
}

/* ------------------------------------------------------------------------- */
/* published order                                                             */
/* ------------------------------------------------------------------------- */
/* the point at position pos of the ring is the next one published */
template <class V>
__device__ __forceinline__ void urf_ring_publish(const V& v, unsigned pos, unsigned* out, unsigned& my_road, unsigned& my_curb)
{
    unsigned cls;
    *out = v.entry(v.at(pos), cls);
    my_road += cls == URF_LABEL_ROAD;
    my_curb += cls == URF_LABEL_CURB;
}
/* ... and the ring's road / curb points for k_ordered_lists (ncls: LDS, zeroed) */
__device__ __forceinline__ void urf_ring_publish_counts(unsigned my_road, unsigned my_curb, unsigned* ncls, unsigned* rcls, unsigned tid)
{
    if (my_road)
        atomicAdd(&ncls[0], my_road);
    if (my_curb)
        atomicAdd(&ncls[1], my_curb);
    __syncthreads();
    if (tid < 2)
        rcls[tid] = ncls[tid];
}

/* Two points of the ring with bit-identical azimuths: their order is the one the reference's Lomuto quicksort
 * (lidar_segmentation.cpp:70-93; deterministic, not stable) leaves.  SORTED = the ring's keys in ascending order; if two neighbours
 * share their azimuth, LIT (the ring's stretch of wsg, which nobody reads after k_star_walk) gets the keys in bucket order -- by
 * position from the view, so SORTED may be LIT itself: it is read before the barrier and written behind it --, one wave runs the
 * quicksort literally (urf_lomuto_sort, as k_nan_rings does for rings with NaN azimuths) and the ring is published in that order.
 * Returns (uniform) whether LIT holds the order.  sh_tie: LDS, zeroed. */
template <unsigned NT, class V>
__device__ __forceinline__ bool urf_ring_literal_order(const V& v, unsigned n, const unsigned long long* SORTED,
                                                       volatile unsigned long long* LIT, unsigned* sh_tie, int* lom_stk, unsigned tid)
{
    for (unsigned j = tid; j + 1 < n; j += NT)
        if ((unsigned)(SORTED[j] >> 32) == (unsigned)(SORTED[j + 1] >> 32))
            *sh_tie = 1u;
    __syncthreads();
    if (!*sh_tie)
        return false;
    for (unsigned j = tid; j < n; j += NT)
        LIT[j] = urf_ring_key(v, j);
    __threadfence_block();
    __syncthreads();
    if (tid < 64)
        urf_lomuto_sort(LIT, n, lom_stk);
    __threadfence_block();
    __syncthreads();
    return true;
}

/* A ring beyond the 2048 points that sort in LDS: bitonic sort of its keys in global memory (G: n entries, may be LIT), ties as above,
 * and the ring published. */
template <unsigned NT, class V>
__device__ __forceinline__ void urf_ring_order_long(const V& v, unsigned n, unsigned long long* G, volatile unsigned long long* LIT,
                                                    unsigned* sh_tie, int* lom_stk, unsigned* rord, unsigned& my_road, unsigned& my_curb,
                                                    unsigned tid)
{
    for (unsigned i = tid; i < n; i += NT)
        G[i] = urf_ring_key(v, i);
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
    const bool lit = urf_ring_literal_order<NT>(v, n, G, LIT, sh_tie, lom_stk, tid);
    for (unsigned j = tid; j < n; j += NT)
        urf_ring_publish(v, lit ? (unsigned)LIT[j] : (unsigned)G[j], &rord[j], my_road, my_curb);
}

/* ------------------------------------------------------------------------- */
/* road_marker: the tables of one ring                                         */
/* ------------------------------------------------------------------------- */
/* Per degree: nrmin = where the scan of this ring stops (the first non-road point: its azimuth bits, or its place in the literal order),
 * best = (d, first in order) of the farthest road point in front of it, bestpos = that point's position in the ring.  In LDS. */
__device__ __forceinline__ int urf_deg_bin(float az)
{
    const int b = (int)__builtin_floorf(az);
    return b < 0 ? 0 : (b > 360 ? 360 : b);
}
struct urf_marker_tabs {
    unsigned long long best[URF_DEG_CELLS];
    int nrmin[URF_DEG_CELLS];
    unsigned bestpos[URF_DEG_CELLS];
    __device__ __forceinline__ void init(unsigned tid)
    {
        for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
            nrmin[i] = URF_INT_NONE_MIN;
            best[i] = 0;
            bestpos[i] = 0xffffffffu;
        }
    }
    /* row c of the scan's tables for k_marker_bins */
    template <class V>
    __device__ __forceinline__ void store(const V& v, unsigned c, float* m_d, unsigned* m_pos, uint8_t* m_red, unsigned tid) const
    {
        for (unsigned i = tid; i < URF_DEG_CELLS; i += 256) {
            const size_t o = (size_t)c * URF_DEG_CELLS + i;
            m_d[o] = __uint_as_float((unsigned)(best[i] >> 32));
            m_pos[o] = bestpos[i] == 0xffffffffu ? 0xffffffffu : v.marker_id(v.at(bestpos[i]));
            m_red[o] = nrmin[i] != URF_INT_NONE_MIN;
        }
    }
};

/* The tables by azimuth, every point looked at pass by pass (T initialised, *need_lit zeroed, a barrier behind both).  need_lit: the
 * ring's ORDER decides (urf_marker_literal). */
template <class V>
__device__ __forceinline__ void urf_marker_passes(const V& v, unsigned n, urf_marker_tabs& T, unsigned* need_lit, unsigned tid)
{
    /* pass 1: where does the scan of this ring stop in each degree (:318) */
    for (unsigned p = tid; p < n; p += 256) {
        const unsigned h = v.at(p), ab = v.az_bits(h);
        const float az = __uint_as_float(ab);
        if ((!V::MAY_NAN || az == az) && v.cls(h) != URF_LABEL_ROAD)
            atomicMin(&T.nrmin[urf_deg_bin(az)], (int)ab);
    }
    __syncthreads();
    /* pass 2: farthest road point in front of it (:325-335); key = (d, first in azimuth order) */
    for (int pass = 0; pass < 2; pass++) {
        for (unsigned p = tid; p < n; p += 256) {
            const unsigned h = v.at(p), ab = v.az_bits(h);
            const float az = __uint_as_float(ab);
            if ((V::MAY_NAN && !(az == az)) || v.cls(h) != URF_LABEL_ROAD)
                continue;
            const int bin = urf_deg_bin(az);
            if ((int)ab == T.nrmin[bin])
                *need_lit = 1u;   /* the very azimuth of the degree's first non-road point: in front of it or behind? */
            if ((int)ab < T.nrmin[bin]) {
                const float d = v.dist(h);
                if (d > 0.0f) {   /* "d > maxDistanceRoad" with maxDistanceRoad starting at 0 */
                    const unsigned long long key = ((unsigned long long)urf_fbits(d) << 32) | (0xffffffffu - ab);
                    if (pass == 0)
                        atomicMax(&T.best[bin], key);
                    else if (key == T.best[bin] && atomicMin(&T.bestpos[bin], p) != 0xffffffffu)
                        *need_lit = 1u;   /* two road points with this distance AND azimuth: which comes first? */
                }
            }
        }
        __syncthreads();
    }
}

/* The same tables when the ring's ORDER decides -- a road point shares its azimuth, bit for bit, with the first non-road point of its
 * degree, or two road points share azimuth and distance: which comes first is what the reference's Lomuto quicksort
 * (lidar_segmentation.cpp:70-93) leaves.  The ring is sorted literally (urf_lomuto_sort on (azimuth, position) pairs in LIT, the ring's
 * stretch of wsg, as k_nan_rings / k_ring_order do) and the three passes compare places in that order instead of azimuths.  Initialises T
 * itself.  Rare: never on a spinning sensor's sweep. */
template <class V>
__device__ __forceinline__ void urf_marker_literal(const V& v, unsigned n, volatile unsigned long long* LIT, urf_marker_tabs& T, int* stk,
                                                   unsigned tid)
{
    T.init(tid);
    for (unsigned p = tid; p < n; p += 256)
        LIT[p] = urf_ring_key(v, p);
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
            const unsigned p = (unsigned)e, h = v.at(p), lab = v.cls(h);
            if (V::MAY_NAN && !(az == az))
                continue;
            const int bin = urf_deg_bin(az);
            if (pass == 0) {
                if (lab != URF_LABEL_ROAD)
                    atomicMin(&T.nrmin[bin], (int)j);   /* :318 the scan of this ring stops here */
            } else if (lab == URF_LABEL_ROAD && (int)j < T.nrmin[bin]) {
                const float d = v.dist(h);
                if (d > 0.0f) {
                    const unsigned long long key = ((unsigned long long)urf_fbits(d) << 32) | (0xffffffffu - j);   /* (d, first in the ring's order) */
                    if (pass == 1)
                        atomicMax(&T.best[bin], key);
                    else if (key == T.best[bin])
                        T.bestpos[bin] = p;
                }
            }
        }
        __syncthreads();
    }
}

/* lidar_segmentation.cpp:305-351 per degree over the nR rings' tables: thread = degree (384 threads, wsum: LDS, one word per wave); the
 * marker points leave in degree order, *count of them. */
template <class V>
__device__ __forceinline__ void urf_marker_bins(const urf_kargs& a, unsigned off, unsigned nR, const float* m_d, const unsigned* m_pos,
                                                const uint8_t* m_red, float* out, unsigned* count, unsigned* wsum)
{
    const unsigned tid = threadIdx.x, wave = tid >> 6;
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
    if (urf_lane() == 0)
        wsum[wave] = __popcll(m);
    __syncthreads();
    unsigned pre = urf_popc_below(m);
    for (unsigned w = 0; w < wave; w++)
        pre += wsum[w];
    if (valid) {
        V::marker_point(a, off, id, out + 4 * pre);
        out[4 * pre + 3] = red;
    }
    if (tid == 0)
        *count = wsum[0] + wsum[1] + wsum[2] + wsum[3] + wsum[4] + wsum[5];
}

#endif /* URF_K_READOUTS_HPP */
