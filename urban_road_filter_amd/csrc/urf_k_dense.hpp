/*
 * urf_k_dense.hpp -- dense sweeps (non-returns dropped by the driver) put back into firing slots by laser id, on the device
 * (urf_classify_batch_soa_dense / urf_classify_batch_pc2_dense, include/urf.h).  One of the kernel families of urf_kernels.hpp;
 * included from there.
 *
 * The rule: point i of a dense scan has slot s_i (its laser id through the slot map); a firing starts at i = 0 and wherever
 * s_i <= s_{i-1}; f_i = firing starts up to and including i, minus 1; the point goes to f_i * L + s_i of a scan of W * L points that is
 * NaN everywhere else.  That position grows strictly with i, so the padded scan holds the dense points in input order with holes between
 * them, which the reference drops before anything else (lidar_segmentation.cpp:100-117): same labels, same counts, for any ids whatever.
 * A scan with a slot >= L or more than W firings is "not aligned": point i stays at position i.
 *
 *   k_dense_count        workgroup (tile of URF_TILE points, scan): firing starts of the tile, bit 31 = a slot >= L was seen
 *   k_dense_scan         workgroup per scan: exclusive prefix over the tiles, the scan's aligned flag, the call's aligned count
 *   k_dense_scatter_*    workgroup (tile, scan): the flags again, prefixed inside the tile (ballot + popcount per wave, the waves joined
 *                        through LDS) on top of the tile's base; x / y / z to the padded staging, the position to the per-point map
 *                        (_pc2 reads the records itself: it stands in for k_pc2_to_soa)
 *   k_dense_labels       d_labels[off[s] + i] = padded labels[s * W * L + pos[i]]
 *   k_dense_ids_*        (urf_classify_batch_*_dense_elev only, in front of the others) the ids themselves, from the points' elevation
 * Positions come from counts and prefixes only.  Point indices inside a scan are 32 bit, everything multiplied by a scan number 64.
 */
#ifndef URF_K_DENSE_HPP
#define URF_K_DENSE_HPP

#define URF_DENSE_THREADS 256
#define URF_DENSE_CHUNKS (URF_TILE / URF_DENSE_THREADS)   /* points per thread: point j * 256 + tid of the tile, j = 0..7 */
#define URF_DENSE_WAVES (URF_DENSE_THREADS / 64)
#define URF_DENSE_BAD 0xffffu        /* the slot of an id the map does not hold */
#define URF_DENSE_BAD_BIT 0x80000000u

struct urf_dense_args {
    const uint32_t* offsets;      /* [n_scans + 1] the caller's */
    uint32_t max_len, n_scans, tiles;   /* tiles per scan = ceil(max_len / URF_TILE): stride of the per-tile words */
    uint32_t L, W;                /* lasers per firing, firings per padded scan */
    const uint8_t* id;            /* the id of point g (index into the caller's arrays) at id + g * id_stride, id_bytes (1 / 2) little-endian */
    uint32_t id_stride, id_bytes;
    const uint8_t* slot_of_id;    /* [256] (0xff: no such id) */
    const float *x, *y, *z;       /* SoA input */
    const uint8_t* data;          /* PointCloud2 input: record g at data + g * step */
    uint32_t step, ox, oy, oz;
    uint32_t* tile_cnt;           /* [n_scans][tiles] */
    uint32_t* tile_base;          /* [n_scans][tiles] */
    uint32_t* aligned;            /* [n_scans] */
    uint32_t* n_aligned;          /* [1] zeroed by the call */
    float *px, *py, *pz;          /* the padded staging: scan s at s * W * L */
    uint32_t* pos;                /* [n_scans][W * L]: position of dense point i inside its padded scan */
    const uint8_t* padded_labels; /* [n_scans][W * L] */
    uint8_t* labels;              /* the caller's, indexed like its points */
};

__device__ __forceinline__ void urf_dense_range(const urf_dense_args& a, unsigned s, unsigned& off, unsigned& len)
{
    off = a.offsets[s];   /* (urf_scan_range: a scan longer than max_len is cut there) */
    len = a.offsets[s + 1] - off;
    len = len > a.max_len ? a.max_len : len;
}

/* slot of point g of the caller's arrays: the id, any alignment, through the map in LDS */
__device__ __forceinline__ unsigned urf_dense_slot(const urf_dense_args& a, const uint8_t* map, unsigned long long g)
{
    const uint8_t* p = a.id + g * a.id_stride;
    unsigned id = p[0];
    if (a.id_bytes == 2u)
        id |= (unsigned)p[1] << 8;
    const unsigned slot = id < 256u ? map[id] : 0xffu;
    return slot < a.L ? slot : URF_DENSE_BAD;
}

/* The tile's slots and firing-start flags: chunk j holds point j * 256 + tid of tile t (i < len), start[j] = the point opens a firing.
 * Returns the mask of chunks whose point exists; `bad` = a slot >= L among this thread's points.  Every thread of the workgroup calls it
 * (the wave shuffles need all lanes). */
__device__ __forceinline__ unsigned urf_dense_flags(const urf_dense_args& a, const uint8_t* map, unsigned off, unsigned len, unsigned t,
                                                    unsigned (&slot)[URF_DENSE_CHUNKS], unsigned& start, bool& bad)
{
    const unsigned tid = threadIdx.x, lane = urf_lane();
    unsigned have = 0;
    start = 0;
    bad = false;
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
        const unsigned i = t * URF_TILE + j * URF_DENSE_THREADS + tid;
        const bool in = i < len;
        slot[j] = in ? urf_dense_slot(a, map, (unsigned long long)off + i) : 0u;
        unsigned prev = (unsigned)__shfl_up((int)slot[j], 1);
        if (lane == 0 && in && i > 0)   /* the point before this wave's first: another wave's, chunk's or tile's */
            prev = urf_dense_slot(a, map, (unsigned long long)off + i - 1u);
        if (in) {
            have |= 1u << j;
            bad = bad || slot[j] == URF_DENSE_BAD;
            if (i == 0 || slot[j] <= prev)
                start |= 1u << j;
        }
    }
    return have;
}

__device__ __forceinline__ void urf_dense_load_map(const urf_dense_args& a, uint8_t* map)
{
    map[threadIdx.x] = a.slot_of_id[threadIdx.x];   /* (URF_DENSE_THREADS == 256 entries) */
    __syncthreads();
}

__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_count(urf_dense_args a)
{
    __shared__ uint8_t map[256];
    __shared__ unsigned sh[URF_DENSE_WAVES];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    urf_dense_load_map(a, map);
    unsigned off, len;
    urf_dense_range(a, s, off, len);
    unsigned slot[URF_DENSE_CHUNKS], start;
    bool bad;
    urf_dense_flags(a, map, off, len, t, slot, start, bad);
    unsigned v = (unsigned)__popc(start) | (bad ? URF_DENSE_BAD_BIT : 0u);   /* (at most 2048 starts per tile: the bit is free) */
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o);
        v = ((v + w) & ~URF_DENSE_BAD_BIT) | ((v | w) & URF_DENSE_BAD_BIT);
    }
    if (urf_lane() == 0)
        sh[wave] = v;
    __syncthreads();
    if (tid == 0) {
        unsigned n = 0, b = 0;
#pragma unroll
        for (unsigned w = 0; w < URF_DENSE_WAVES; w++) {
            n += sh[w] & ~URF_DENSE_BAD_BIT;
            b |= sh[w] & URF_DENSE_BAD_BIT;
        }
        a.tile_cnt[(size_t)s * a.tiles + t] = n | b;
    }
}

/* per scan: the tiles' first firing, the scan's firing count against W, the bad-slot bits */
__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_scan(urf_dense_args a)
{
    __shared__ unsigned wsum[URF_DENSE_WAVES], wbad[URF_DENSE_WAVES];
    const unsigned s = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = urf_lane();
    const size_t row = (size_t)s * a.tiles;
    unsigned carry = 0, bad = 0;
    for (unsigned t0 = 0; t0 < a.tiles; t0 += URF_DENSE_THREADS) {
        const unsigned t = t0 + tid;
        const unsigned w = t < a.tiles ? a.tile_cnt[row + t] : 0u;
        const unsigned n = w & ~URF_DENSE_BAD_BIT;
        bad |= w & URF_DENSE_BAD_BIT;
        const unsigned incl = urf_wave_incl(n);
        if (lane == 63)
            wsum[wave] = incl;
        __syncthreads();
        unsigned before = carry, all = 0;
#pragma unroll
        for (unsigned k = 0; k < URF_DENSE_WAVES; k++) {
            before += k < wave ? wsum[k] : 0u;
            all += wsum[k];
        }
        if (t < a.tiles)
            a.tile_base[row + t] = before + incl - n;
        carry += all;
        __syncthreads();
    }
    const unsigned long long anybad = __ballot(bad != 0u);
    if (lane == 0)
        wbad[wave] = anybad != 0ull ? 1u : 0u;
    __syncthreads();
    if (tid == 0) {
        unsigned b = 0;
#pragma unroll
        for (unsigned k = 0; k < URF_DENSE_WAVES; k++)
            b |= wbad[k];
        const unsigned ok = (b == 0u && carry <= a.W) ? 1u : 0u;
        a.aligned[s] = ok;
        if (ok)
            atomicAdd(a.n_aligned, 1u);
    }
}

template <bool PC2>
__device__ __forceinline__ void urf_dense_scatter(const urf_dense_args& a)
{
    __shared__ uint8_t map[256];
    __shared__ unsigned cnt[URF_DENSE_CHUNKS * URF_DENSE_WAVES];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = urf_lane();
    urf_dense_load_map(a, map);
    unsigned off, len;
    urf_dense_range(a, s, off, len);
    if (t * URF_TILE >= len)   /* (uniform: nothing of this tile exists) */
        return;
    unsigned slot[URF_DENSE_CHUNKS], start;
    bool bad;
    const unsigned have = urf_dense_flags(a, map, off, len, t, slot, start, bad);
    /* firing starts in input order: chunk j, wave w, lane -- counts per (j, w), then the starts at or before this lane */
    unsigned incl[URF_DENSE_CHUNKS];
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
        const unsigned long long m = __ballot(((start >> j) & 1u) != 0u);
        incl[j] = (unsigned)__popcll(m & (~0ull >> (63u - lane)));
        if (lane == 0)
            cnt[j * URF_DENSE_WAVES + wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    const bool aligned = a.aligned[s] != 0u;
    const unsigned WL = a.W * a.L;
    const unsigned long long pbase = (unsigned long long)s * WL;
    unsigned run = a.tile_base[(size_t)s * a.tiles + t];   /* firing starts before this (chunk, wave) */
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
#pragma unroll
        for (unsigned w = 0; w < URF_DENSE_WAVES; w++) {
            const unsigned c = cnt[j * URF_DENSE_WAVES + w];
            if (w == wave && ((have >> j) & 1u)) {
                const unsigned i = t * URF_TILE + j * URF_DENSE_THREADS + tid;
                const unsigned long long g = (unsigned long long)off + i;
                /* (aligned: run + incl >= 1, the scan's first point opens firing 0; f < W and slot < L, so p < W * L) */
                const unsigned p = aligned ? (run + incl[j] - 1u) * a.L + slot[j] : i;
                float fx, fy, fz;
                if (PC2) {
                    const uint8_t* r = a.data + g * a.step;
                    if ((((unsigned long long)(r + a.ox) | (unsigned long long)(r + a.oy) | (unsigned long long)(r + a.oz)) & 3ull) == 0) {
                        fx = *(const float*)(r + a.ox);
                        fy = *(const float*)(r + a.oy);
                        fz = *(const float*)(r + a.oz);
                    } else {   /* (k_pc2_to_soa's unaligned path) */
                        unsigned bx = 0, by = 0, bz = 0;
                        for (int b = 3; b >= 0; b--) {
                            bx = (bx << 8) | r[a.ox + b];
                            by = (by << 8) | r[a.oy + b];
                            bz = (bz << 8) | r[a.oz + b];
                        }
                        fx = __uint_as_float(bx);
                        fy = __uint_as_float(by);
                        fz = __uint_as_float(bz);
                    }
                } else {
                    fx = a.x[g];
                    fy = a.y[g];
                    fz = a.z[g];
                }
                if (p < WL) {   /* (always: max_len <= W * L, and see above) */
                    a.px[pbase + p] = fx;
                    a.py[pbase + p] = fy;
                    a.pz[pbase + p] = fz;
                    a.pos[pbase + i] = p;
                }
            }
            run += c;
        }
    }
}

__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_scatter_soa(urf_dense_args a) { urf_dense_scatter<false>(a); }
__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_scatter_pc2(urf_dense_args a) { urf_dense_scatter<true>(a); }

__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_labels(urf_dense_args a)
{
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    unsigned off, len;
    urf_dense_range(a, s, off, len);
    const unsigned WL = a.W * a.L;
    const unsigned long long pbase = (unsigned long long)s * WL;
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
        const unsigned i = t * URF_TILE + j * URF_DENSE_THREADS + tid;
        if (i < len) {
            const unsigned p = a.pos[pbase + i];
            a.labels[(unsigned long long)off + i] = p < WL ? a.padded_labels[pbase + p] : (uint8_t)0;
        }
    }
}

/* ---- the way back: the reference-order lists of the padded batch in the caller's dense indices (urf_set_dense_outputs) -------------
 * pos grows strictly with i inside a scan, so its inverse is a function on the positions that hold a point; the ordered lists
 * (k_ordered_lists) hold only such positions, the holes being NaN and dropped before anything else.
 *   k_dense_inverse      workgroup (tile, scan): inv[s * W * L + pos[i]] = i for the scan's points; the holes of inv are never written
 *   k_dense_unmap_lists  workgroup (256 entries, scan, list): entries 0 .. count - 1 of road / curb / ring10 in place, p -> inv[p];
 *                        every entry is checked against pos (a hole of inv holds anything), a miss stores URF_DENSE_NONE */
#define URF_DENSE_NONE 0xffffffffu

struct urf_dense_unmap_args {
    const uint32_t* offsets;      /* [n_scans + 1] the context's copy of the dense call's */
    uint32_t max_len, WL;         /* the dense call's; W * L: stride of pos and inv */
    const uint32_t* pos;          /* [n_scans][W * L] */
    uint32_t* inv;                /* [n_scans][W * L] */
};

__device__ __forceinline__ void urf_dense_unmap_range(const urf_dense_unmap_args& a, unsigned s, unsigned& len)
{
    len = a.offsets[s + 1] - a.offsets[s];   /* (urf_dense_range) */
    len = len > a.max_len ? a.max_len : len;
}

__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_inverse(urf_dense_unmap_args a)
{
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    unsigned len;
    urf_dense_unmap_range(a, s, len);
    const unsigned long long pbase = (unsigned long long)s * a.WL;
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
        const unsigned i = t * URF_TILE + j * URF_DENSE_THREADS + tid;
        if (i < len) {   /* (len <= max_len <= W * L: inside the scan's row of pos) */
            const unsigned p = a.pos[pbase + i];
            if (p < a.WL)
                a.inv[pbase + p] = i;
        }
    }
}

/* scans [s0, s0 + gridDim.y) of the dense call; the lists and counts as k_ordered_lists wrote them (scan s0 first, a list may be NULL) */
__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_unmap_lists(urf_dense_unmap_args a, unsigned s0, unsigned* road_all,
                                                                         unsigned* curb_all, unsigned* ring10_all, unsigned stride,
                                                                         const unsigned* counts_all)
{
    const unsigned k = blockIdx.z, s = s0 + blockIdx.y;
    const unsigned e = blockIdx.x * URF_DENSE_THREADS + threadIdx.x;
    unsigned* const all = k == 0 ? road_all : k == 1 ? curb_all : ring10_all;
    if (!all)
        return;
    unsigned n = counts_all[(size_t)blockIdx.y * 3 + k];
    n = n > stride ? stride : n;
    if (e >= n)
        return;
    unsigned len;
    urf_dense_unmap_range(a, s, len);
    const unsigned long long pbase = (unsigned long long)s * a.WL;
    unsigned* const q = all + (size_t)blockIdx.y * stride + e;
    const unsigned p = *q;
    unsigned i = URF_DENSE_NONE;
    if (p < a.WL) {
        const unsigned j = a.inv[pbase + p];
        if (j < len && a.pos[pbase + j] == p)
            i = j;
    }
    *q = i;
}

/* ---- laser ids from elevation, for clouds without a `ring` field (urf_classify_batch_*_dense_elev, include/urf.h) -------------------
 * The caller's table of elevations per firing slot, ranked on the host (urf_set_dense_elevations): thr[k] = the tangent of the midpoint
 * between the k-th and the (k+1)-th ranked elevation, slot_of_rank[r] = the slot of rank r.  Per point h = sqrtf(x * x + y * y), rank =
 * the number of k with z > thr[k] * h, id = slot_of_rank[rank].  thr[k] * h does not decrease with k (thr does not, h >= 0, and a
 * rounded product keeps the order), so the compares are true up to the rank and false from there on: a binary search, 7 steps over the
 * 127 entries of a table padded with +Inf (z > Inf * h is false for every z and h, NaN included).  What the compares give for
 * non-finite points, (0, 0, 0) and points on the axis is the rule; nothing downstream depends on an id being right.
 *   k_dense_ids_*        workgroup (tile, scan): one id byte per point to ids[offsets[s] + i], indexed like the caller's arrays -- where
 *                        k_dense_count and k_dense_scatter_* then read them (id_stride 1, id_bytes 1, the identity map of the table) */
#define URF_DENSE_ELEV_MAX 128

/* what urf_set_dense_elevations builds and the elevation calls copy to the device (dn_elev), as it lies there */
struct urf_dense_elev_table {
    float thr[URF_DENSE_ELEV_MAX];                 /* [n - 1] ascending, +Inf behind them */
    uint8_t slot_of_rank[URF_DENSE_ELEV_MAX];      /* [n] */
    uint8_t identity[256];                         /* the slot map of derived ids: urf_set_dense_slots' does not apply to them */
};

struct urf_dense_ids_args {
    const urf_dense_elev_table* table;
    uint8_t* ids;                 /* [cap] */
    unsigned long long cap;       /* bytes of ids: a point at or beyond it (offsets the context was not made for) is not written */
};

template <bool PC2>
__device__ __forceinline__ void urf_dense_ids(const urf_dense_args& a, const urf_dense_ids_args& e)
{
    __shared__ float thr[URF_DENSE_ELEV_MAX];
    __shared__ uint8_t sor[URF_DENSE_ELEV_MAX];
    const unsigned t = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    unsigned off, len;
    urf_dense_range(a, s, off, len);
    if (t * URF_TILE >= len)   /* (uniform: nothing of this tile exists) */
        return;
    if (tid < URF_DENSE_ELEV_MAX) {
        thr[tid] = e.table->thr[tid];
        sor[tid] = e.table->slot_of_rank[tid];
    }
    __syncthreads();
#pragma unroll
    for (unsigned j = 0; j < URF_DENSE_CHUNKS; j++) {
        const unsigned i = t * URF_TILE + j * URF_DENSE_THREADS + tid;
        const unsigned long long g = (unsigned long long)off + i;
        if (i >= len || g >= e.cap)
            continue;
        float fx, fy, fz;
        if (PC2) {   /* (k_dense_scatter_pc2's two ways to a record) */
            const uint8_t* r = a.data + g * a.step;
            if ((((unsigned long long)(r + a.ox) | (unsigned long long)(r + a.oy) | (unsigned long long)(r + a.oz)) & 3ull) == 0) {
                fx = *(const float*)(r + a.ox);
                fy = *(const float*)(r + a.oy);
                fz = *(const float*)(r + a.oz);
            } else {
                unsigned bx = 0, by = 0, bz = 0;
                for (int b = 3; b >= 0; b--) {
                    bx = (bx << 8) | r[a.ox + b];
                    by = (by << 8) | r[a.oy + b];
                    bz = (bz << 8) | r[a.oz + b];
                }
                fx = __uint_as_float(bx);
                fy = __uint_as_float(by);
                fz = __uint_as_float(bz);
            }
        } else {
            fx = a.x[g];
            fy = a.y[g];
            fz = a.z[g];
        }
        const float h = sqrtf(fx * fx + fy * fy);
        unsigned rank = 0;
#pragma unroll
        for (unsigned step = URF_DENSE_ELEV_MAX / 2; step > 0; step >>= 1)   /* thr[rank + step - 1] <= thr[126] */
            if (fz > thr[rank + step - 1u] * h)
                rank += step;
        e.ids[g] = sor[rank];   /* (rank <= n - 1: the padding compares false) */
    }
}

__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_ids_soa(urf_dense_args a, urf_dense_ids_args e) { urf_dense_ids<false>(a, e); }
__global__ __launch_bounds__(URF_DENSE_THREADS) void k_dense_ids_pc2(urf_dense_args a, urf_dense_ids_args e) { urf_dense_ids<true>(a, e); }

#endif /* URF_K_DENSE_HPP */
