/*
 * urf_k_clouds.hpp -- the four published clouds of a batch as device-resident pcl::PointXYZI records
 * (urf_clouds_batch_soa / urf_clouds_batch_pc2, include/urf.h).  One of the kernel families of urf_kernels.hpp; included from there.
 *
 * lidar_segmentation.cpp:354-367, 605-608, 620 copy whole pcl::PointXYZI records into "road", "curb", "roi" and "road_probably".
 * Here that is a streaming compaction over the label bytes of the last batch call, in four launches:
 *   k_clouds_count    workgroup (tile, scan): the tile's four counts (labels as 16-byte vectors, SWAR, wave + LDS reduction),
 *                     one uint4 per (scan, tile), no atomics; a scan whose status is not URF_OK counts nothing
 *   k_clouds_scan     workgroup per scan: exclusive prefix over its tiles (per-tile bases inside the scan) and the scan's counts
 *   k_clouds_offsets  one workgroup: exclusive prefix over (scan, cloud) in 64 bits -> the clouds' record offsets
 *   k_clouds_write    workgroup (tile, scan): ranks by ballot + mbcnt and a prefix across the waves, every point's source read once,
 *                     its 32-byte record stored to each of its clouds as two 16-byte stores (consecutive ranks: contiguous memory)
 * and, for the reference's order, k_clouds_gather behind k_ring_order / k_ordered_lists (urf_ordered_indices_batch's kernels):
 * thread i of a cloud reads entry i of the ordered list and writes record i.  Positions come from counts and prefixes only:
 * layout and values do not depend on scheduling.
 */
#ifndef URF_K_CLOUDS_HPP
#define URF_K_CLOUDS_HPP

#define URF_CLOUDS_COUNT_THREADS 128   /* 16 labels per thread: one tile */
#define URF_CLOUDS_THREADS 256
/* where the points' x / y / z / intensity come from (urf_clouds_args::src) */
#define URF_SRC_SOA 0u        /* the SoA call's x / y / z, intensity from a separate array (or 0) */
#define URF_SRC_PC2 1u        /* PointCloud2 records, every field dword-aligned */
#define URF_SRC_PC2_BYTES 2u  /* ... any point_step / offsets / base: byte loads (k_pc2_to_soa's unaligned path) */
#define URF_SRC_PC2_XYZ 3u    /* ... x y z at 0 / 4 / 8 of 16-byte aligned records: one 16-byte load (+ intensity) */

typedef unsigned urf_u32x4 __attribute__((ext_vector_type(4)));

struct urf_clouds_args {
    const uint8_t* labels;        /* the last call's */
    const uint32_t* offsets;      /* ragged: [n_scans + 1] (context copy); else NULL */
    const urf_scan_info* info;    /* the context's per-scan results of that call */
    uint32_t n_per_scan, max_len, tiles, n_scans;
    const unsigned* x;            /* URF_SRC_SOA: the values as bits */
    const unsigned* y;
    const unsigned* z;
    const unsigned* in;           /* NULL: intensity 0 */
    const uint8_t* data;          /* URF_SRC_PC2*: record i at data + i * step */
    uint32_t step, ox, oy, oz;
    int32_t oi;                   /* -1: no intensity field */
    uint32_t src;                 /* URF_SRC_* */
    urf_u32x4* tile_cnt;          /* [n_scans][tiles] road, curb, roi, road_probably */
    urf_u32x4* tile_base;         /* [n_scans][tiles] the same, exclusive prefix over the scan's tiles */
    uint32_t* counts;             /* [4 * n_scans] (caller's) */
    unsigned long long* offs;     /* [4 * n_scans] (caller's) */
    urf_u32x4* rec;               /* two per record (caller's); NULL: counts and offsets only */
    const uint32_t* lists;        /* reference order: [3][n_scans][stride] road, curb, road_probably (k_ordered_lists) */
    const uint32_t* list_cnt;     /* [n_scans][3] */
    uint32_t stride;
};

__device__ __forceinline__ void urf_clouds_range(const urf_clouds_args& a, unsigned s, unsigned& off, unsigned& len)
{
    if (a.offsets) {   /* (urf_scan_range: a scan longer than max_len is cut there) */
        off = a.offsets[s];
        len = a.offsets[s + 1] - off;
        len = len > a.max_len ? a.max_len : len;
    } else {
        off = s * a.n_per_scan;
        len = a.n_per_scan;
    }
}

/* four label bytes -> (road | curb << 16, roi | road_probably << 16) of them */
__device__ __forceinline__ void urf_clouds_swar(unsigned w, unsigned& rc, unsigned& ri)
{
    const unsigned road = w & ~(w >> 1) & 0x01010101u;   /* (label & 3) == 1 */
    const unsigned curb = (w >> 1) & ~w & 0x01010101u;   /* (label & 3) == 2 */
    rc += (unsigned)__popc(road) | ((unsigned)__popc(curb) << 16);
    ri += (unsigned)__popc((w >> 2) & 0x01010101u) | ((unsigned)__popc((w >> 4) & 0x01010101u) << 16);
}

__global__ __launch_bounds__(URF_CLOUDS_COUNT_THREADS) void k_clouds_count(urf_clouds_args a)
{
    __shared__ unsigned sh[URF_CLOUDS_COUNT_THREADS / 64][2];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    unsigned off, len;
    urf_clouds_range(a, s, off, len);
    const unsigned i0 = t * URF_TILE;
    unsigned rc = 0, ri = 0;   /* 16-bit fields: at most 2048 per tile */
    if (a.info[s].status == URF_OK && i0 < len) {
        const unsigned n = len - i0 < URF_TILE ? len - i0 : URF_TILE;
        const uint8_t* L = a.labels + off + i0;
        const unsigned j = tid * 16u;
        if (j + 16u <= n && ((uintptr_t)(L + j) & 15u) == 0) {
            const urf_u32x4 w = *(const urf_u32x4*)(L + j);
            urf_clouds_swar(w.x, rc, ri);
            urf_clouds_swar(w.y, rc, ri);
            urf_clouds_swar(w.z, rc, ri);
            urf_clouds_swar(w.w, rc, ri);
        } else if (j < n) {   /* the scan's last partial vector, or labels of a ragged scan that start off a 16-byte boundary */
#pragma unroll
            for (unsigned q = 0; q < 4; q++) {
                unsigned w = 0;
#pragma unroll
                for (unsigned b = 0; b < 4; b++)
                    if (j + 4 * q + b < n)
                        w |= (unsigned)L[j + 4 * q + b] << (8 * b);
                urf_clouds_swar(w, rc, ri);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rc += __shfl_xor(rc, o);
        ri += __shfl_xor(ri, o);
    }
    if (urf_lane() == 0) {
        sh[wave][0] = rc;
        sh[wave][1] = ri;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned r = 0, i = 0;
#pragma unroll
        for (unsigned w = 0; w < URF_CLOUDS_COUNT_THREADS / 64; w++) {
            r += sh[w][0];
            i += sh[w][1];
        }
        urf_u32x4 c;
        c.x = r & 0xffffu;
        c.y = r >> 16;
        c.z = i & 0xffffu;
        c.w = i >> 16;
        a.tile_cnt[(size_t)s * a.tiles + t] = c;
    }
}

/* inclusive prefix over the lanes of a wave */
__device__ __forceinline__ unsigned urf_wave_incl(unsigned v)
{
    const unsigned lane = urf_lane();
#pragma unroll
    for (unsigned o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o);
        v += lane >= o ? u : 0u;
    }
    return v;
}

/* per scan: the tiles' bases inside the scan, the scan's four counts */
__global__ __launch_bounds__(URF_CLOUDS_THREADS) void k_clouds_scan(urf_clouds_args a)
{
    constexpr unsigned NW = URF_CLOUDS_THREADS / 64;
    __shared__ unsigned wsum[NW][4];
    const unsigned s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const size_t row = (size_t)s * a.tiles;
    unsigned carry[4] = { 0, 0, 0, 0 };
    for (unsigned t0 = 0; t0 < a.tiles; t0 += URF_CLOUDS_THREADS) {
        const unsigned t = t0 + tid;
        urf_u32x4 v = { 0, 0, 0, 0 };
        if (t < a.tiles)
            v = a.tile_cnt[row + t];
        const unsigned val[4] = { v.x, v.y, v.z, v.w };
        unsigned inc[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            inc[k] = urf_wave_incl(val[k]);
            if (urf_lane() == 63)
                wsum[wave][k] = inc[k];
        }
        __syncthreads();
        unsigned ex[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            unsigned pre = carry[k], tot = 0;
#pragma unroll
            for (unsigned w = 0; w < NW; w++) {
                pre += w < wave ? wsum[w][k] : 0u;
                tot += wsum[w][k];
            }
            ex[k] = pre + inc[k] - val[k];
            carry[k] += tot;
        }
        if (t < a.tiles) {
            urf_u32x4 b;
            b.x = ex[0];
            b.y = ex[1];
            b.z = ex[2];
            b.w = ex[3];
            a.tile_base[row + t] = b;
        }
        __syncthreads();
    }
    if (tid < 4)
        a.counts[(size_t)s * 4 + tid] = carry[tid];
}

/* one workgroup: d_offsets = exclusive prefix of d_counts over (scan, cloud), in 64 bits */
#define URF_CLOUDS_OFF_THREADS 1024
__global__ __launch_bounds__(URF_CLOUDS_OFF_THREADS) void k_clouds_offsets(urf_clouds_args a)
{
    constexpr unsigned NW = URF_CLOUDS_OFF_THREADS / 64;
    __shared__ unsigned long long wsum[NW];
    const unsigned tid = threadIdx.x, wave = tid >> 6;
    const size_t m = (size_t)a.n_scans * 4;
    unsigned long long carry = 0;
    for (size_t b = 0; b < m; b += URF_CLOUDS_OFF_THREADS) {
        const size_t i = b + tid;
        const unsigned v = i < m ? a.counts[i] : 0u;
        const unsigned inc = urf_wave_incl(v);   /* 64 counts of at most max_points (< 2^23) each: fits */
        if (urf_lane() == 63)
            wsum[wave] = inc;
        __syncthreads();
        unsigned long long pre = carry, tot = 0;
#pragma unroll
        for (unsigned w = 0; w < NW; w++) {
            pre += w < wave ? wsum[w] : 0ull;
            tot += wsum[w];
        }
        if (i < m)
            a.offs[i] = pre + inc - v;
        carry += tot;
        __syncthreads();
    }
}

/* point i of the last call's inputs (index into the caller's arrays / records): (x, y, z, 1.0f) and (intensity, 0, 0, 0), bit for bit */
__device__ __forceinline__ void urf_clouds_point(const urf_clouds_args& a, unsigned i, urf_u32x4& lo, urf_u32x4& hi)
{
    unsigned x, y, z, in = 0;
    if (a.src == URF_SRC_SOA) {
        x = a.x[i];
        y = a.y[i];
        z = a.z[i];
        if (a.in)
            in = a.in[i];
    } else {
        const uint8_t* p = a.data + (size_t)i * a.step;
        if (a.src == URF_SRC_PC2_XYZ) {
            const urf_u32x4 v = *(const urf_u32x4*)p;
            x = v.x;
            y = v.y;
            z = v.z;
            if (a.oi == 12)
                in = v.w;
            else if (a.oi >= 0)
                in = *(const unsigned*)(p + a.oi);
        } else if (a.src == URF_SRC_PC2) {
            x = *(const unsigned*)(p + a.ox);
            y = *(const unsigned*)(p + a.oy);
            z = *(const unsigned*)(p + a.oz);
            if (a.oi >= 0)
                in = *(const unsigned*)(p + a.oi);
        } else {
            x = y = z = 0;
            for (int b = 3; b >= 0; b--) {
                x = (x << 8) | p[a.ox + b];
                y = (y << 8) | p[a.oy + b];
                z = (z << 8) | p[a.oz + b];
            }
            if (a.oi >= 0)
                for (int b = 3; b >= 0; b--)
                    in = (in << 8) | p[a.oi + b];
        }
    }
    lo.x = x;
    lo.y = y;
    lo.z = z;
    lo.w = 0x3f800000u;   /* w = 1.0f (pcl::PointXYZI's data[3]) */
    hi.x = in;
    hi.y = hi.z = hi.w = 0u;
}

template <bool NT>
__device__ __forceinline__ void urf_clouds_store(urf_u32x4* rec, unsigned long long pos, const urf_u32x4& lo, const urf_u32x4& hi)
{
    urf_u32x4* q = rec + 2 * pos;
    if (NT) {
        __builtin_nontemporal_store(lo, q);
        __builtin_nontemporal_store(hi, q + 1);
    } else {
        q[0] = lo;
        q[1] = hi;
    }
}

/* input order.  which: bit k = cloud k is written here (0xf; 0x4 = roi only, when the others come in the reference's order) */
template <bool NT>
__global__ __launch_bounds__(URF_CLOUDS_THREADS) void k_clouds_write(urf_clouds_args a, unsigned which)
{
    constexpr unsigned NW = URF_CLOUDS_THREADS / 64;
    __shared__ unsigned wsum[2][4][NW];   /* double-buffered by round: one barrier per round */
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (a.info[s].status != URF_OK)
        return;   /* (its counts are 0) */
    unsigned off, len;
    urf_clouds_range(a, s, off, len);
    const unsigned i0 = t * URF_TILE;
    if (i0 >= len)
        return;
    const unsigned n = len - i0 < URF_TILE ? len - i0 : URF_TILE;
    const uint8_t* L = a.labels + off + i0;
    const urf_u32x4 tb = a.tile_base[(size_t)s * a.tiles + t];
    const unsigned long long* so = a.offs + (size_t)s * 4;
    const unsigned long long base[4] = { so[0] + tb.x, so[1] + tb.y, so[2] + tb.z, so[3] + tb.w };
    unsigned run[4] = { 0, 0, 0, 0 };
    for (unsigned r = 0; r * URF_CLOUDS_THREADS < n; r++) {
        const unsigned j = r * URF_CLOUDS_THREADS + tid;
        const unsigned f = j < n ? urf_label_classes(L[j]) & which : 0u;   /* bit 0 road, 1 curb, 2 roi, 3 road_probably */
        unsigned below[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long m = __ballot((f >> k) & 1u);
            below[k] = urf_popc_below(m);
            if (lane == 0)
                wsum[r & 1][k][wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
        unsigned pos[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pos[k] = run[k] + below[k];
#pragma unroll
            for (unsigned w = 0; w < NW; w++) {
                const unsigned c = wsum[r & 1][k][w];
                pos[k] += w < wave ? c : 0u;
                run[k] += c;
            }
        }
        if (f) {
            urf_u32x4 lo, hi;
            urf_clouds_point(a, off + i0 + j, lo, hi);
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((f >> k) & 1u)
                    urf_clouds_store<NT>(a.rec, base[k] + pos[k], lo, hi);
        }
    }
}

/* reference order: road, curb, road_probably (blockIdx.z = 0, 1, 2 -> clouds 0, 1, 3) from the ordered lists */
template <bool NT>
__global__ __launch_bounds__(URF_CLOUDS_THREADS) void k_clouds_gather(urf_clouds_args a)
{
    const unsigned k = blockIdx.z, cl = k == 2 ? 3u : k, s = blockIdx.y;
    const unsigned i = blockIdx.x * URF_CLOUDS_THREADS + threadIdx.x;
    const unsigned c0 = a.counts[(size_t)s * 4 + cl], c1 = a.list_cnt[(size_t)s * 3 + k];
    if (i >= (c0 < c1 ? c0 : c1))
        return;
    unsigned off, len;
    urf_clouds_range(a, s, off, len);
    const unsigned src = a.lists[((size_t)k * a.n_scans + s) * a.stride + i];
    if (src >= len)
        return;   /* (cannot happen) */
    urf_u32x4 lo, hi;
    urf_clouds_point(a, off + src, lo, hi);
    urf_clouds_store<NT>(a.rec, a.offs[(size_t)s * 4 + cl] + i, lo, hi);
}

#endif /* URF_K_CLOUDS_HPP */
