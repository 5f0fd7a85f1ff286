/*
 * urf_front.hpp -- the fused front end for organised sweeps (r6): firing by firing, or row-major (height = the lasers) through k_transpose.
 *
 * What it replaces: k_split + k_ring (+ k_label's ring-sorted reads) for a scan whose points come as a spinning
 * LiDAR's driver delivers them -- firing after firing, every firing holding the sensor's 64 lasers in ONE fixed order
 * (elevation order, laser-number order, any permutation), points missing where there was no return or the region of
 * interest cut them off (lidar_segmentation.cpp:100-117), the points of a firing that take part in the star-shaped
 * search sharing one sector (star_shaped_search.cpp:164-171).
 *
 * The legacy path sorts every tile by ring so that a workgroup per ring can stream its points (k_split: 39 B/point,
 * k_ring: 7 B/point more).  Here LANE l of a wave IS laser l: the wave marches along the firings of its block, 64
 * points (one firing) per step, coalesced 256-byte loads per array, and the lane keeps the last 2 * curbPoints + 1 points of
 * ITS ring in registers -- the window both detectors look at, eleven points for curbPoints == 5 (x_zero_method.cpp:30-67: the triple
 * (j, j + 2, j + 5); z_zero_method.cpp:21-72: the centre and five points on either side).  A lane whose point is
 * missing simply does not shift its window: a hole costs nothing and needs no compaction.  Nothing is sorted by ring,
 * nothing is transposed, x / y / z are read once and only the 4-byte record (input order) and the star-shaped search's
 * sector-sorted copies leave the kernel: 26 B/point instead of 46.
 *
 *   k_front        grid (blocks of URF_FRONT tiles, scans) x 64 threads.  Per step: region of interest, ring (the
 *                  lane's expected table entry first, the reference's exact sequence for the rare point that is not
 *                  surely on it), sector, azimuth code, the cheap height tests of both detectors for the point whose
 *                  window has just become complete; what passes goes to the scan's candidate list.  Per tile: the
 *                  sector run table k_index and the sort kernels read (tsoff), the presence word of every lane.
 *                  A block starts URF_FRONT_HPRE firings early and ends URF_FRONT_HPOST firings late (windows
 *                  across block borders); what a hole in the halo leaves undecided goes to the list as an EDGE item.
 *   k_front_finish one workgroup per scan, behind the star-shaped search: ring sizes and positions from the presence
 *                  words, the angle tests of the candidates (f64 chains, all lanes busy), the star-shaped hits, the
 *                  rings' curb lists, largest ranges and quadrants for k_beams.
 *   k_label_front  k_label in input order: record -> label byte, no LDS image.
 *   k_transpose    (row-major organised sweeps: point l * F + f, front_ok[s] == URF_FRONT_ROWS, decided by k_rows_probe + k_ring_table,
 *                  urf_k_table.hpp) the firing-order copy of x / y / z the three kernels above read instead of the caller's arrays;
 *                  everything between input and output is indexed by firing * 64 + laser, k_label_front stores the labels row-major
 *                  and k_star_ties (urf_k_star.hpp) ranks a sector in the reference's row order before it re-enacts std::sort.
 *
 * A scan that does not have the shape (a lane that meets two rings, two lanes on one ring, a firing in two sectors,
 * sectors that fall inside a tile, a ring point on the sensor's axis, an incomplete speculative ring table) clears
 * front_ok[s] and takes the legacy kernels, which skip every scan whose flag is still set.  Labels are the same
 * either way, bit for bit: the arithmetic is the legacy path's (urf_device.hpp, urf_x_zero_angle, urf_z_zero_angle).
 * With urf_set_front_multi_sector on, "a firing in two sectors" and "sectors that fall inside a tile" are no such reasons (the star-shaped
 * search on; curbPoints 5, and 1..4 and 6..8 with urf_set_front_multi_sector_curb_points on top): the march is a k_front*_ms or
 * k_front*_ms_cp<n> instance (urf_front_body's MS) and k_front_sectors (urf_k_front_sectors.hpp) sorts each tile's star records by sector
 * behind it.
 *
 * ONE body per kernel around the march, for every laser count.  k_front_finish*, k_transpose (here) and k_rows_probe (urf_k_table.hpp) each
 * exist as a named wrapper per family -- 64 / 32 / 16 lasers, the count read at run time, and 128 (k_front_finish128*, k_transpose128,
 * k_rows_probe128), the count a constant -- around urf_front_finish_body<CP, W128>, urf_transpose_body<W128>, urf_rows_probe_body<W128>.  What
 * differs between the families (the arrays and their strides, the hand-over words of front_st, the record's ring field) stands in
 * urf_front_lay<W128>; the code differs in how the finish adds up a scan's ring points, under `if constexpr`.  k_label_front128 is still a copy
 * of k_label_front (see there: folded, both lose 6 registers and 1 - 2.6 % of their time to the wrapper).
 *
 * ONE march body.  urf_front_body<STAR, BEAM, L, CP> is every k_front* -- 64, 32 and 16 lasers, one per lane, and 128 (k_front128*,
 * behind urf_set_front_lasers128), two per lane: the body holds its per-laser state as urf_front_ring<CP> R[NH], NH = 1 or 2 halves of a
 * firing, and writes down once what else the laser count decides (see there; profiles/front_one_body.md).  CP = params.curbPoints, 1..8, and
 * 5 -- k_front, k_front32, k_front16, k_front128, the symbols of every front mode -- is an instance like the other seven
 * (URF_FRONT_CP_OTHERS: the fused front modes 3 and urf_set_front_curb_points).  What depends on CP lives in urf_front_window<CP>: the 2 CP + 1
 * heights, the packed firing numbers, the detectors' height tests.  Until that layout the body for 5 was a copy with eleven named registers,
 * because "with CP as a parameter" k_front had come out with 96 registers and a spill.  The parameter was not the cause: named scalars,
 * arrays and a struct of arrays give the same code.  The cause is the few lines of the block-end tail (URF_FRONT_TAIL_CALLS), which tip the
 * register allocation of the whole function one way or the other; tests/test_kernel_resources.py and its siblings hold every instance to
 * its register budget and to no scratch, so a change that tips it back fails there.
 */
#ifndef URF_FRONT_HPP
#define URF_FRONT_HPP

#include "urf_policy.hpp"

#define URF_FRONT_HPRE 8u      /* firings in front of a block: 7 fill a window without holes (x_zero's j >= 5 rule) */
#ifndef URF_FRONT_HPRE_WIDE
#define URF_FRONT_HPRE_WIDE 12u   /* ... for curbPoints 6..8 (mode 3): the point x_zero marks needs CP + CP / 2 = 9, 10, 12 ring points in front of it */
#endif
#ifndef URF_FRONT_HPOST
#define URF_FRONT_HPOST 8u     /* firings behind it: 5 complete the last centre's window */
#endif
#define URF_FRONT_LANES 64u
#define URF_FRONT_STEPS (URF_TILE / URF_FRONT_LANES)   /* firings per tile */
/* (What only the host's decision reads -- batch thresholds, tiles per block, URF_FRONT_CP_OTHERS, tile limits, URF_FRONT128_TILES2 -- stands in urf_policy.hpp.) */
#define URF_FRONT_CP_MASK 0x1feu   /* urf_policy.hpp's, repeated to the letter: tests/test_front_curb_points_resources.py reads it here */
#define URF_FRONT_RING_NONE 0x7fu  /* ring field of an input-order record */
#define URF_FRONT_ST_WORDS 72u   /* k_front_finish part 1 -> part 2: 64 list lengths, 4 quadrant values, the length of the list of marks, two counts */
/* ... and of the 128-laser family (urf_set_front_lasers128), whose arrays are the siblings sized for 128 (urf_kargs::*128), allocated when
 * the switch is turned on.  What these kernels leave behind keeps the layout its readers know, indexed by f * 128 + l: region-of-interest bits
 * (two 64-bit words per firing), slots (stp * 128 + l < 2048), tsoff, candidate indices.  A tile is 16 firings and a presence word 32 of
 * them: word (f >> 5) * 128 + l covers two tiles, so the words per scan are counted for an even number of tiles (URF_FRONT128_TILES2), and a
 * block of the march holds an even number of tiles (front_tpb, urf_policy.hpp) -- no presence word is shared between two blocks. */
#define URF_FRONT128_L 128u
#define URF_FRONT128_LSH 7u
#define URF_FRONT128_RING_MASK 0xffu   /* ring field of an input-order record of these kernels: table entry 127 is a ring, 0xff is "none" */
#define URF_FRONT128_RING_NONE 0xffu
#define URF_FRONT128_ST_WORDS 136u     /* k_front_finish128 part 1 -> part 2: 128 list lengths, 4 quadrant values, list length, two counts */
/* candidate kinds */
#define URF_FC_XZ 1u       /* passed x_zero's height tests as the marked point: angle test pending */
#define URF_FC_ZZ 2u       /* passed z_zero's as the centre */
#define URF_FC_EDGE_X 4u   /* x_zero not evaluated by the march (window incomplete at a block border): everything pending */
#define URF_FC_EDGE_Z 8u
#ifndef URF_FRONT_NT
#define URF_FRONT_NT 0   /* cache policy of k_front's stores (2 = non-temporal).  A sweep with drop-outs compacts its star records, a step's 64 stores then straddle
                          * cache lines that the next step completes: non-temporal, such half-written lines left the L2 at once (the address queue in
                          * front of it full 18 x as often as on a sweep without holes, k_front 1.50 ms per 1024 sensor-like sweeps against 0.98) */
#endif
#ifndef URF_FRONT_WAVES
#define URF_FRONT_WAVES 5   /* 88 registers; at 6 (80) the kernel reloads a spilled constant in every step, behind an s_waitcnt vmcnt(0) that drains its prefetch */
#endif

struct urf_front_thr {
    float y, z, below;   /* (an entry the table does not hold: y = +inf, nothing lies inside) */
};
__device__ __forceinline__ urf_front_thr urf_front_load_thr(const urf_kargs& a, unsigned s, unsigned C, unsigned e, unsigned nR)
{
    urf_front_thr t;
    const bool valid = e < nR;
    const float4 tv = ((const float4*)a.ring_thr)[(size_t)s * C + (valid ? e : 0u)];
    const float bl = a.ring_thr[((size_t)s * C + ((valid && e) ? e - 1u : 0u)) * 4];
    t.y = valid ? tv.y : __builtin_inff();
    t.z = tv.z;
    t.below = e ? bl : __builtin_inff();
    return t;
}

/* raw buffer descriptors (gfx9 word 3: 32-bit untyped): a lane whose byte offset lies at or beyond `bytes` loads zero and stores
 * nothing -- the march's loads behind the scan's end and its predicated stores need neither a select nor a branch, and the
 * compiler sees a straight line of memory operations (its s_waitcnt for the points loaded four firings ago then leaves every
 * younger operation in flight: loads and stores share ONE in-order counter on this chip, and a wait that cannot count the stores
 * in between waits for all of them -- the first version of this kernel spent two thirds of its time there) */
__device__ __forceinline__ __amdgpu_buffer_rsrc_t urf_buf(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)bytes, 0x00020000);
}
#define URF_OOB 0xffffffffu

/* the arrays the fused kernels read a scan's points from, indexed by firing * 64 + laser: the caller's for a sweep in firing order,
 * k_transpose's copy for a row-major one (front_ok[s] == URF_FRONT_ROWS) */
__device__ __forceinline__ void urf_front_src(const urf_kargs& a, unsigned s, unsigned off, unsigned ok, const float*& gx, const float*& gy, const float*& gz)
{
    const bool rows = ok == URF_FRONT_ROWS;   /* (uniform) */
    const size_t o = rows ? (size_t)urf_sbase(a, s) : (size_t)off;
    gx = (rows ? (const float*)a.tx : a.x) + o;
    gy = (rows ? (const float*)a.ty : a.y) + o;
    gz = (rows ? (const float*)a.tz : a.z) + o;
}

/* The laser layout of a fused scan: what the kernels around the march have to know about the two families.  W128 = false is 64, 32 or 16
 * lasers per firing, the count read at run time (front_lsh), the arrays sized for 64 lanes; W128 = true is 128 lasers, the count a constant,
 * the arrays the siblings sized for 128.  Outside of this struct the difference is known to the two marches, which write the arrays, and to
 * the rows' probe (urf_k_table.hpp: included in front of this header, it picks rows_v / rows_v128 itself). */
template <bool W128>
struct urf_front_lay {
    static constexpr unsigned NL = W128 ? URF_FRONT128_L : URF_FRONT_LANES;   /* the ARRAYS' lasers per scan (the firing's: L) */
    static constexpr unsigned RING_MASK = W128 ? URF_FRONT128_RING_MASK : 0x7fu;   /* ring field of an input-order record ... */
    static constexpr unsigned RING_NONE = W128 ? URF_FRONT128_RING_NONE : URF_FRONT_RING_NONE;   /* ... and its "on no ring" */
    /* front_st, part 1 -> part 2 of the finish kernel: the curb lists' lengths per laser slot from word 0 on, then */
    static constexpr unsigned ST_QUAD = NL, ST_NPEND = NL + 4u, ST_RING_PTS = NL + 5u, ST_RING10 = NL + 6u;
    static constexpr unsigned ST_WORDS = W128 ? URF_FRONT128_ST_WORDS : URF_FRONT_ST_WORDS;
    static_assert(ST_RING10 < ST_WORDS, "the hand-over words fit");

    /* L = 1 << lsh lasers per firing */
    static __device__ __forceinline__ unsigned lsh(const urf_kargs& a)
    {
        if constexpr (W128)
            return URF_FRONT128_LSH;
        else
            return a.front_lsh;
    }
    /* the tiles the presence words and the blocks' maxima are counted for */
    static __device__ __forceinline__ unsigned tiles(const urf_kargs& a)
    {
        if constexpr (W128)
            return URF_FRONT128_TILES2(a.tiles);
        else
            return a.tiles;
    }
    /* the scan's presence words: word (f >> 5) * L + l */
    static __device__ __forceinline__ uint32_t* pres(const urf_kargs& a, unsigned s)
    {
        return (W128 ? a.front_pres128 : a.front_pres) + (size_t)s * tiles(a) * 64u;
    }
    /* the largest x * x + y * y of every laser slot in block `b` of the march: NL values, written there, read by the finish */
    static __device__ __forceinline__ unsigned long long* maxs_of_block(const urf_kargs& a, unsigned s, unsigned b)
    {
        if constexpr (W128)
            return a.front_maxs128 + (size_t)s * tiles(a) * 64u + (size_t)b * NL;
        else
            return a.front_maxs + ((size_t)s * a.tiles + b) * 64u;
    }
    static __device__ __forceinline__ unsigned long long maxs(const urf_kargs& a, unsigned s, unsigned b, unsigned l)
    {
        return maxs_of_block(a, s, b)[l];
    }
    static __device__ __forceinline__ uint32_t* lane_ring(const urf_kargs& a, unsigned s)
    {
        return (W128 ? a.front_lane_ring128 : a.front_lane_ring) + (size_t)s * NL;
    }
    static __device__ __forceinline__ uint32_t* st(const urf_kargs& a, unsigned s)
    {
        return (W128 ? a.front_st128 : a.front_st) + (size_t)s * ST_WORDS;
    }
};
/* ... for a kernel that serves both families (the read-outs, urf_k_front_outputs.hpp): the family from front_lsh */
__device__ __forceinline__ const uint32_t* urf_front_pres_of(const urf_kargs& a, unsigned s)
{
    return a.front_lsh == URF_FRONT128_LSH ? urf_front_lay<true>::pres(a, s) : urf_front_lay<false>::pres(a, s);
}
__device__ __forceinline__ const uint32_t* urf_front_lane_ring_of(const urf_kargs& a, unsigned s)
{
    return a.front_lsh == URF_FRONT128_LSH ? urf_front_lay<true>::lane_ring(a, s) : urf_front_lay<false>::lane_ring(a, s);
}

/* Row-major organised sweep of L = 1 << lsh rows -> firing order: tx[f * L + l] = x[l * F + f].  Grid (tiles, scans) x 256 threads, a tile =
 * URF_TILE / L firings: L rows x 64 / 128 / 256 / 512 bytes in, LDS, 8 KB out in one stretch; 24 B/point, HBM-bound. */
template <bool W128>
__device__ __forceinline__ void urf_transpose_body(urf_kargs a)
{
    using LAY = urf_front_lay<W128>;
    /* [row][W + 1], W = URF_TILE / L columns: 64 x 33 (and in it 32 x 65, 16 x 129), 128 x 17.  (128 x 17: a wave stores four rows x 16 columns
     * -- addresses 17 r + c: 64 different ones over a span of 67, three banks twice -- and reads 64 rows of one column: stride 17, odd, no
     * conflict) */
    __shared__ float T[3][LAY::NL * (URF_TILE / LAY::NL + 1u)];
    const unsigned s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const unsigned lsh = LAY::lsh(a), L = 1u << lsh, wsh = 11u - lsh, W = 1u << wsh, RS = W + 1u;
    static_assert(URF_TILE == 2048u, "a tile's columns: 1 << (11 - lsh)");
    if (a.front_ok[s] != URF_FRONT_ROWS)
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned F = len >> lsh, f0 = t * W;
    if (f0 >= F)
        return;
    const unsigned c = tid & (W - 1u), r8 = tid >> wsh, RP = 256u >> wsh;   /* RP rows per pass, eight passes: L rows */
    const bool in = f0 + c < F;
    float vx[8], vy[8], vz[8];
#pragma unroll
    for (unsigned j = 0; j < 8; j++) {
        const size_t i = (size_t)off + (size_t)(j * RP + r8) * F + f0 + (in ? c : 0u);
        vx[j] = a.x[i];
        vy[j] = a.y[i];
        vz[j] = a.z[i];
    }
#pragma unroll
    for (unsigned j = 0; j < 8; j++) {
        T[0][(j * RP + r8) * RS + c] = vx[j];
        T[1][(j * RP + r8) * RS + c] = vy[j];
        T[2][(j * RP + r8) * RS + c] = vz[j];
    }
    __syncthreads();
    const size_t ob = (size_t)urf_sbase(a, s) + (size_t)f0 * L;
    const unsigned nf = F - f0 < W ? F - f0 : W;
#pragma unroll
    for (unsigned j = 0; j < 8; j++) {
        const unsigned v = j * 256u + tid, f = v >> lsh, l = v & (L - 1u);
        if (f < nf) {
            a.tx[ob + v] = T[0][l * RS + f];
            a.ty[ob + v] = T[1][l * RS + f];
            a.tz[ob + v] = T[2][l * RS + f];
        }
    }
}
__global__ __launch_bounds__(256) void k_transpose(urf_kargs a)
{
    urf_transpose_body<false>(a);
}
__global__ __launch_bounds__(256) void k_transpose128(urf_kargs a)
{
    urf_transpose_body<true>(a);
}

/* What the fast decisions of a firing leave open -- a point that is not SURELY on its lane's table entry, whose sector is within
 * the margin of a border, or that the approximations refuse: the reference's exact sequence (urf_exact_keys).  Returns bit 0: on
 * the lane's ring; bits 1-11: sector + 1 (0: none wanted); bits 12-18 + URF_FO_ADOPT: the lane has no confirmed entry yet and the
 * point lies on this one; URF_FO_NONE: on no ring; URF_FO_FAIL: the scan does not have the shape (one lane, two rings; a ring point
 * on the sensor's axis, whose azimuth is NaN: k_nan_rings, legacy path).  NOT inlined: a call under a branch that is rarely
 * taken, and nothing the hot path keeps in registers depends on what happens in here. */
#define URF_FO_ADOPT 0x20000000u
#define URF_FO_NONE 0x40000000u
#define URF_FO_FAIL 0x80000000u
__device__ __noinline__ unsigned urf_front_open(const float* tab, unsigned nR, float interval, float x, float y, float z, unsigned sectors, float Kfi,
                                                unsigned E, unsigned econf)
{
    const urf_exact_key ek = urf_exact_keys_body(tab, nR, interval, x, y, z, sectors, Kfi);
    unsigned r = sectors ? ((ek.sector + 1u) & 0x7ffu) << 1 : 0u;
    if (ek.ring == URF_RING_NONE)
        r |= URF_FO_NONE;
    else if (x == 0.0f && y == 0.0f)
        r |= URF_FO_FAIL;
    else if (ek.ring == E)
        r |= 1u;
    else if (!econf)
        r |= 1u | URF_FO_ADOPT | (ek.ring << 12);
    else
        r |= URF_FO_FAIL;
    return r;
}

/* the wave's candidate buffer (LDS; the workgroup IS the wave) and its flush into the scan's list: one atomic per ~150 candidates */
#define URF_FRONT_CBUF 256u
/* max(|v[I]|, |v[I + S]|, ..., N operands) as the chain of v_max3_f32 the march has always used (window values are region-of-interest
 * points' heights, never NaN: |.| modifiers, no quieting): three operands first, two more per instruction, a last single one with v_max_f32.
 * Every index is a compile-time constant: the window stays in registers. */
template <unsigned N, int I, int S, unsigned NW>
__device__ __forceinline__ float urf_front_absmax_more(float t, const float (&v)[NW])
{
    if constexpr (N == 0u) {
        return t;
    } else if constexpr (N == 1u) {
        float m;
        asm("v_max_f32_e64 %0, %1, |%2|" : "=v"(m) : "v"(t), "v"(v[I]));
        return m;
    } else {
        asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(t) : "v"(t), "v"(v[I]), "v"(v[I + S]));
        return urf_front_absmax_more<N - 2u, I + 2 * S, S>(t, v);
    }
}
template <unsigned N, int I, int S, unsigned NW>
__device__ __forceinline__ float urf_front_absmax(const float (&v)[NW])
{
    static_assert(N >= 2u, "the centre and at least one neighbour");
    float t;
    if constexpr (N == 2u) {
        asm("v_max_f32_e64 %0, |%1|, |%2|" : "=v"(t) : "v"(v[I]), "v"(v[I + S]));
        return t;
    } else {
        asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(t) : "v"(v[I]), "v"(v[I + S]), "v"(v[I + 2 * S]));
        return urf_front_absmax_more<N - 3u, I + 3 * S, S>(t, v);
    }
}
__device__ __forceinline__ void urf_front_flush(const urf_kargs& a, unsigned s, urf_u2* cbuf, unsigned& ncb, bool& overflow)
{
    if (ncb == 0u)
        return;   /* (uniform) */
    urf_wave_lds_sync();
    unsigned base = 0;
    if (urf_lane() == 0u)
        base = atomicAdd(&a.front_ncand[s], ncb);
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    for (unsigned j = urf_lane(); j < ncb; j += 64u) {
        if (base + j < a.front_cand_cap)
            a.front_cand[(size_t)s * a.front_cand_cap + base + j] = cbuf[j];
        else
            overflow = true;
    }
    urf_wave_lds_sync();
    ncb = 0;
}
__device__ __forceinline__ void urf_front_push(urf_u2* cbuf, unsigned& ncb, bool has, unsigned idx, unsigned what)
{
    const unsigned long long m = __ballot(has);
    if (has)
        cbuf[ncb + urf_popc_below(m)] = urf_u2{ idx, what };
    ncb += (unsigned)__popcll(m);
}

/* The window of one laser (urf_front_body: one per lane, two at 128 lasers).  CP = params.curbPoints, H = CP / 2.  It holds the laser's last 2 * CP + 1 ring points, w[2 * CP] the newest: z_zero's centre is w[CP] (CP points
 * on either side, z_zero_method.cpp:21-50), x_zero's triple (j, j + H, j + CP) is (w[CP], w[CP + H], w[2 * CP]) and the point it marks the
 * one CP - H back (x_zero_method.cpp:30-34; CP == 1: the triple is (j, j, j + 1)).  Both loops start at j = CP: a decision needs the FULL
 * window.  fw[] keeps the firing numbers (relative to the march's first firing) of the newest CP + 1 points, 16 bits each, the newest in
 * the upper half of the last register: the point `back` places behind it sits in half 2 * NFW - 1 - back.  Every index below is a
 * constant once the loops are unrolled: registers. */
template <unsigned CP>
struct urf_front_window {
    static_assert(CP >= 1u && CP <= 8u && URF_FRONT_HPOST >= CP, "the halo behind a block completes the last centre's window");
    static constexpr unsigned H = CP / 2u, NW = 2u * CP + 1u, NFW = (CP + 2u) / 2u;
    static constexpr unsigned HPRE = CP <= 5u ? URF_FRONT_HPRE : URF_FRONT_HPRE_WIDE;   /* CP + H ring points in front of a block's first marked point */
    /* (the counters in front of the arrays: in the other order k_front128 needs a register more and k_front128_cp7 spills) */
    unsigned wc;                           /* points in the window, at most NW */
    unsigned tot, nin;                     /* ring points of this laser since the block's first firing / inside the block */
    unsigned fw[NFW];                      /* (CP == 5: (f6 << 16 | f5), (f8 << 16 | f7), (f10 << 16 | f9)) */
    float w[NW];

    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (unsigned k = 0; k < NW; k++)
            w[k] = 0.f;
#pragma unroll
        for (unsigned k = 0; k < NFW; k++)
            fw[k] = 0u;
        wc = tot = nin = 0u;
    }
    /* a new ring point, met in firing `fr` of the march; PH: urf_front_body's phase */
    template <unsigned PH>
    __device__ __forceinline__ void push(const float z, const unsigned fr)
    {
#pragma unroll
        for (unsigned k = 0; k + 1u < NW; k++)
            w[k] = w[k + 1u];
        w[NW - 1u] = z;
#pragma unroll
        for (unsigned k = 0; k + 1u < NFW; k++)
            fw[k] = __builtin_amdgcn_alignbit(fw[k + 1u], fw[k], 16);
        fw[NFW - 1u] = __builtin_amdgcn_alignbit(fr, fw[NFW - 1u], 16);
        wc = wc < NW ? wc + 1u : NW;
        if (PH >= 1u)
            tot++;
        if (PH == 1u)
            nin++;
    }
    __device__ __forceinline__ bool full() const { return wc == NW; }
    /* the centre (CP points back) and the point x_zero marks (CP - H back): are they this block's */
    __device__ __forceinline__ bool c_in(const bool on) const { return on & (tot >= CP + 1u) & (tot - CP <= nin); }
    __device__ __forceinline__ bool p_in(const bool on) const { return on & (tot >= CP - H + 1u) & (tot - (CP - H) <= nin); }
    /* ... and the point `back` places behind the newest */
    __device__ __forceinline__ bool in_block(const unsigned back) const { return tot > back && tot - back <= nin; }
    /* z_zero_method.cpp:39-40, 48-49, 67-69.  (Window values are region-of-interest points' heights, never NaN: v_max3 with |.| modifiers,
     * three instructions per side for CP == 5 -- the compiler's fmaxf quiets the first two operands of every chain with a v_max x, x each: five) */
    __device__ __forceinline__ bool hz(const float curbH) const
    {
        const float a5 = __builtin_fabsf(w[CP]);
        const float m1 = urf_front_absmax<CP + 1u, 0, 1>(w);                 /* the CP older points, then the centre */
        const float m2 = urf_front_absmax<CP + 1u, (int)(2u * CP), -1>(w);   /* the CP newer points from the newest on, then the centre */
        return ((m1 - a5 >= curbH) | (m2 - a5 >= curbH)) & (__builtin_fabsf(m1 - m2) >= 0.05f);   /* ((double)v >= 0.05 <=> v >= 0.05f: the float above 0.05) */
    }
    /* x_zero_method.cpp:62-64 for the triple (w[CP], w[CP + H], w[2 CP]) = (j, j + H, j + CP) */
    __device__ __forceinline__ bool hx(const float curbH) const
    {
        return ((__builtin_fabsf(w[CP] - w[CP + H]) >= curbH) | (__builtin_fabsf(w[2u * CP] - w[CP + H]) >= curbH)) & (__builtin_fabsf(w[CP] - w[2u * CP]) >= 0.05f);
    }
    /* firing of the point `back` places behind the newest, of the centre, of the point x_zero marks */
    __device__ __forceinline__ unsigned firing(const unsigned back) const
    {
        const unsigned sl = 2u * NFW - 1u - back;
        return (sl & 1u) ? fw[sl / 2u] >> 16 : fw[sl / 2u] & 0xffffu;
    }
    __device__ __forceinline__ unsigned centre_firing() const { return firing(CP); }
    __device__ __forceinline__ unsigned marked_firing() const { return firing(CP - H); }
};

/* The block-end tail of the march: tail(CP - 1), ..., tail(0), each index a std::integral_constant, written out as calls of a NAMED
 * lambda.  The form of these few lines decides the code of the WHOLE march at curbPoints 5 and 64 / 32 / 16 lanes: as a `#pragma unroll`
 * loop (over an array of firing numbers taken out of fw[] first, or over firing(back)), or handed to a helper template that does the
 * counting, k_front comes out with 96 registers, a 16-byte spill and 380 more v_mov_b32; like this with 92 and none.
 * profiles/front_one_march.md has the table. */
#define URF_FRONT_TAIL_CALLS(CP, tail)                                         \
    if constexpr ((CP) >= 8u) tail(std::integral_constant<unsigned, 7u>{});    \
    if constexpr ((CP) >= 7u) tail(std::integral_constant<unsigned, 6u>{});    \
    if constexpr ((CP) >= 6u) tail(std::integral_constant<unsigned, 5u>{});    \
    if constexpr ((CP) >= 5u) tail(std::integral_constant<unsigned, 4u>{});    \
    if constexpr ((CP) >= 4u) tail(std::integral_constant<unsigned, 3u>{});    \
    if constexpr ((CP) >= 3u) tail(std::integral_constant<unsigned, 2u>{});    \
    if constexpr ((CP) >= 2u) tail(std::integral_constant<unsigned, 1u>{});    \
    tail(std::integral_constant<unsigned, 0u>{});

/* what the march keeps per laser.  (Keep the members' order: it decides a spill at 128 lasers, profiles/front_one_march.md) */
template <unsigned CP>
struct urf_front_ring {
    unsigned E;          /* the table entry this laser's points are expected on */
    bool econf;          /* ... and a point of this march has confirmed it */
    urf_front_thr th;
    urf_front_window<CP> win;   /* its last 2 * CP + 1 ring points, firings relative to Fs */
    double maxs;         /* largest x*x + y*y among its ring points of the block (maxDistance, lidar_segmentation.cpp:271-274) */
    unsigned pw;         /* presence bits of the 32 firings at hand */
};

/* The march.  L = the lasers of a firing (params.channels: 128, 64, 32, 16).  Point f * L + l is laser slot l of firing f: everything the march leaves
 * behind -- records, region-of-interest bits, the sector-sorted copies and their slots, candidate indices -- is indexed by the point's place in
 * the input, a tile is URF_TILE points = URF_TILE / L firings, and k_index and the star-shaped search read a scan of any L alike.  Only
 * the presence words count in firings: word (f >> 5) * L + l.  CP = params.curbPoints, 1..8: 5 is an instance like the others
 * (urf_front_window).
 *
 * ONE wave per block, whatever L is, and a lane marches NH lasers: laser h * 64 + lane for h < NH, the HALVES of a firing.  For L < 64 the
 * lanes from L on are idle (no point, never in the region of interest): one march per wave, the chain of a block URF_TILE / L steps per tile.
 * For L = 128 a firing is two wave-widths, NH = 2: lane j marches lasers j and j + 64, with two windows and two sets of per-ring state
 * (R[NH]).  The two halves of a firing are worked off back to back inside one step, so that everything that crosses lanes -- the slot rank
 * of a star participant, the one-sector test, the step's key and count -- spans the 128 lasers in input order with two ballots and no LDS
 * traffic or barrier, and the candidate buffer stays "the workgroup is the wave".  The price is registers.  Every
 * array of NH below is indexed by constants only (the loops over h are unrolled): registers, and for NH = 1 the code of scalars.
 *
 * What the laser count decides besides NH is named here once: the arrays sized for 64 or for 128 lanes and the record's "on no ring"
 * (urf_front_lay<(L > 64)>), the width of a firing's region-of-interest word (step), which half the first star participant comes from and
 * how many there are in front of a half (step), how many registers hold a tile's steps (NK).
 *
 * MS (urf_set_front_multi_sector; k_front*_ms, and k_front*_ms_cp<n> behind urf_set_front_multi_sector_curb_points; STAR only, any CP -- nothing
 * below that depends on MS reads the window): a firing's participants may lie in SEVERAL sectors, and the sectors may
 * fall inside a tile -- a real sensor's azimuth offsets per laser, its rotation during a firing, the sweep's seam.  The march then leaves
 * the tile's star records compacted in INPUT order as ever (tile base + participants in front), each with its 16-bit sector in the same
 * place of front_skey, and the tile's participant count in tsoff[row][K]; k_front_sectors (urf_k_front_sectors.hpp) sorts the tile's
 * records by sector, stably, and writes the tile's tsoff row.  No one-sector test, no step keys, no bisection; every other rule stays. */
template <bool STAR, bool BEAM, unsigned L, unsigned CP, bool MS = false>
__device__ __forceinline__ void urf_front_body(const urf_kargs& a, const urf_dev_params& dp, urf_u2* cbuf)
{
    static_assert(L == 128u || L == 64u || L == 32u || L == 16u, "a firing fills two waves, the wave, half of it or a quarter");
    static_assert(!MS || STAR, "multi-sector needs the star-shaped search");
    using LAY = urf_front_lay<(L > 64u)>;
    constexpr unsigned NH = L > 64u ? 2u : 1u;    /* halves of a firing: lasers per lane */
    const unsigned s = blockIdx.y, b = blockIdx.x, lane = threadIdx.x;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned TPB = a.front_tpb;   /* (128 lasers: even, urf_policy.hpp -- no presence word is shared between two blocks) */
    const unsigned t_first = b * TPB;
    if (t_first * URF_TILE >= len)
        return;
    const unsigned ok = a.front_ok[s];
    if (ok == 0u)
        return;
    constexpr unsigned C = L;                     /* table entries per scan: params.channels */
    constexpr unsigned STEPS = URF_TILE / L;      /* firings per tile */
    constexpr unsigned W = STEPS < 64u ? STEPS : 64u, NK = STEPS / W;   /* a tile's steps: NK registers, W lanes of each */
    constexpr unsigned H = urf_front_window<CP>::H, HPRE = urf_front_window<CP>::HPRE;
    const unsigned K = (unsigned)dp.p.sectors;
    const unsigned nf = (len + L - 1u) / L;                                 /* firings of the scan */
    const unsigned F0 = t_first * STEPS;
    const unsigned F1 = F0 + TPB * STEPS < nf ? F0 + TPB * STEPS : nf;
    const unsigned Fs = F0 > HPRE ? F0 - HPRE : 0u;
    const unsigned Fe = F1 + URF_FRONT_HPOST < nf ? F1 + URF_FRONT_HPOST : nf;
    const bool from_start = Fs == 0u;   /* the window count IS the ring position + 1 */
    const bool to_end = Fe == nf;       /* no point of the scan lies behind the march */
    static_assert(HPRE % 4u == 0u && STEPS % 4u == 0u, "the march runs in groups of four firings");
    const unsigned sb = urf_sbase(a, s);
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, ok, gx, gy, gz);
    const __amdgpu_buffer_rsrc_t brec = urf_buf(a.rec + sb, len * 4u);
    const __amdgpu_buffer_rsrc_t bsr = urf_buf(a.sr + sb, a.tiles * URF_TILE * 4u), bsz = urf_buf(a.sz + sb, a.tiles * URF_TILE * 4u);
    const __amdgpu_buffer_rsrc_t bss = urf_buf(a.sslot + sb, a.tiles * URF_TILE * 2u);
    const __amdgpu_buffer_rsrc_t bsk = MS ? urf_buf(a.front_skey + sb, a.tiles * URF_TILE * 2u) : bss;   /* (MS: the records' sectors, slot for slot) */
    const unsigned nR = a.info[s].n_rings;
    const unsigned upto_v = a.table_upto[s];
    /* (a row-major scan's table rests on EVERY point lying on its row's entry -- k_ring_table's third rule: a point on none asks for the long walk) */
    const unsigned upto = ok == URF_FRONT_ROWS ? 0u : (nR < C ? upto_v : 0xffffffffu);
    const float* const tab = a.angle + (size_t)s * dp.p.channels;
    const float curbH = dp.p.curbHeight;
    const bool use_x = dp.p.x_zero_method != 0, use_z = dp.p.z_zero_method != 0;
    const bool mine = L >= 64u || lane < L;   /* this lane has a laser */
    const unsigned mylen = mine ? len : 0u;   /* ... and to a lane that has none the scan is empty: one compare where a point is looked at */

    urf_front_ring<CP> R[NH];
#pragma unroll
    for (unsigned h = 0; h < NH; h++) {
        R[h].E = h * 64u + lane;
        R[h].econf = false;
        R[h].th = urf_front_load_thr(a, s, C, R[h].E, nR);
        R[h].win.clear();
        R[h].maxs = 0.0;
        R[h].pw = 0u;
    }
    bool failed = false, overflow = false;
    unsigned long long failed_m = 0;   /* ... what the hot path finds wrong, as lane masks (wave-uniform) */
    unsigned ncb = 0;                  /* candidates in the wave's buffer */
    /* per tile (wave-uniform) */
    unsigned troi = 0, tstar = 0;
    int stepkey_v[NK], stepcnt_v[NK];   /* register q, lane j < W: sector / participating points of step q * 64 + j of the tile */
#pragma unroll
    for (unsigned q = 0; q < NK; q++) {
        stepkey_v[q] = (int)URF_SEC_NONE;
        stepcnt_v[q] = 0;
    }

    /* one firing.  PH 0: the halo in front of the block (windows fill), 1: the block, 2: the halo behind it (windows complete) */
    auto step = [&](auto ph, const unsigned f, const float (&X)[NH], const float (&Y)[NH], const float (&Z)[NH]) {
        constexpr unsigned PH = decltype(ph)::value;
        const unsigned stp = f % STEPS;
        bool roi[NH], on[NH];
        unsigned long long roim[NH], roi_any = 0ull;
#pragma unroll
        for (unsigned h = 0; h < NH; h++) {
            roi[h] = f * L + h * 64u + lane < mylen && urf_in_roi(dp.p, X[h], Y[h], Z[h]);
            roim[h] = __ballot(roi[h]);
            roi_any |= roim[h];
        }
        if (PH == 1u && lane < NH) {   /* bit i of the scan's words: input point i.  A firing is ... */
            if constexpr (NH > 1u) {         /* ... two 64-bit words, written by two lanes */
                a.roi_bits[((size_t)s * a.tiles + f / STEPS) * (URF_TILE / 64u) + stp * NH + lane] = lane ? roim[NH - 1u] : roim[0];
            } else if constexpr (L == 64u) {   /* ... one */
                a.roi_bits[((size_t)s * a.tiles + f / STEPS) * (URF_TILE / 64u) + stp] = roim[0];
            } else {                         /* ... half or a quarter of one */
                using word_t = std::conditional_t<L == 32u, uint32_t, uint16_t>;
                ((word_t*)(a.roi_bits + (size_t)s * a.tiles * (URF_TILE / 64u)))[f] = (word_t)roim[0];
            }
        }
        if (roi_any == 0ull)
            return;   /* (uniform) nothing of this firing lies in the region of interest */
        float rho2[NH], fi[NH];
        unsigned sk[NH];
        bool ons[NH];
        unsigned long long psm[NH];
#pragma unroll
        for (unsigned h = 0; h < NH; h++) {
            urf_front_ring<CP>& r = R[h];
            const float x = X[h], y = Y[h], z = Z[h];
            const unsigned i = f * L + h * 64u + lane;
            rho2[h] = x * x + y * y;
            const float u = -z * __builtin_amdgcn_rsqf(rho2[h]);   /* urf_fast_cot */
            const bool fast = (rho2[h] >= URF_FAST_MIN2) & (rho2[h] <= URF_FAST_MAX2) & (__builtin_fabsf(u) <= URF_LUT_UMAX) & roi[h];
            const bool on_f = fast & (u >= r.th.y) & (u <= r.th.z) & (u < r.th.below);
            fi[h] = 0.f;
            int fs = -1;
            if (PH == 1u) {
                fi[h] = urf_fast_polar(x, y);
                if (STAR)
                    fs = fast ? urf_fast_sector_ranged(fi[h], dp.Kfi, K, dp.sector_margin) : -1;
            }
            on[h] = on_f;
            const bool open = roi[h] && !(on_f && (PH != 1u || !STAR || fs >= 0));
            /* (r6, vector-issue diet: a ballot of anything but a direct compare costs two vector instructions -- v_cndmask 0 / 1, v_cmp -- to
             * mask it with exec; a plain divergent branch skips its block when no lane takes it for two SCALAR instructions.  Wave-level
             * flags (failed, overflow) are OR-ed up as masks, per-lane state that only rare paths read (econf) likewise.) */
            if (open) {   /* rare: the reference's exact sequence for the lanes that need it */
                const unsigned o = urf_front_open(tab, nR, dp.p.interval, x, y, z, (PH == 1u && STAR) ? K : 0u, dp.Kfi, r.E, r.econf ? 1u : 0u);
                on[h] = (o & 1u) != 0u;
                fs = (int)((o >> 1) & 0x7ffu) - 1;
                if (o & URF_FO_FAIL)
                    failed = true;
                if (PH == 1u && (o & URF_FO_NONE) && i >= upto)
                    a.table_redo[s] = 1u;   /* the speculative ring table is incomplete (k_table_repair, legacy path) */
                if (o & URF_FO_ADOPT) {   /* this laser sits on another table entry: learned from its first point */
                    r.E = (o >> 12) & 0x7fu;
                    r.th = urf_front_load_thr(a, s, C, r.E, nR);
                }
            }
            sk[h] = (unsigned)fs;
            ons[h] = false;
            psm[h] = 0ull;
            if (PH == 1u) {
                /* the record, input order: ring | azimuth code (URF_REC_*; detector hits are OR-ed in by k_front_finish) */
                const unsigned azc_v = urf_az_code(urf_fast_azimuth_of(fi[h]));   /* (unconditionally, then a select: a branch around eight instructions costs more) */
                const unsigned azc = urf_fast_az_ok(x, y) ? azc_v : URF_REC_AZ_UNKNOWN;
                __builtin_amdgcn_raw_buffer_store_b32((azc << URF_REC_AZ_SHIFT) | (on[h] ? r.E : LAY::RING_NONE), brec, mine ? i * 4u : URF_OOB, 0, URF_FRONT_NT);
                if (STAR) {
                    if (BEAM && roi[h] && !urf_in_beam(a.beams[fs < 0 ? 0 : fs], x, y))
                        sk[h] = URF_SEC_NONE;
                    /* (every lane is active here: the masks of direct compares need no exec) */
                    psm[h] = roim[h] & __builtin_amdgcn_ballot_w64(sk[h] != URF_SEC_NONE) & __builtin_amdgcn_ballot_w64((int)sk[h] >= 0);
                    ons[h] = roi[h] && sk[h] != URF_SEC_NONE && (int)sk[h] >= 0;
                    /* (outside the interval of urf_sqrt_rn_normal's shortcut: the legacy kernels) */
                    failed_m |= psm[h] & ~(__builtin_amdgcn_ballot_w64(rho2[h] >= 0x1p-90f) & __builtin_amdgcn_ballot_w64(rho2[h] <= 0x1p126f));
                }
            }
        }
        if (PH == 1u) {
            if (STAR) {
                /* star-shaped search: the firing's participants -- of every half -- share one sector, the first participant's (half 0's, or
                 * else half 1's), and their copies follow each other in input order: half 0's, then half 1's */
                unsigned f0 = URF_SEC_NONE;
                if constexpr (!MS) {
#pragma unroll
                    for (unsigned h = NH; h-- > 0u;) {
                        const unsigned src = psm[h] ? (unsigned)__ffsll((long long)psm[h]) - 1u : 0u;
                        f0 = psm[h] ? (unsigned)__builtin_amdgcn_readlane((int)sk[h], (int)src) : f0;
                    }
                }
                unsigned np = 0;   /* participants of the halves in front */
#pragma unroll
                for (unsigned h = 0; h < NH; h++) {
                    if constexpr (!MS)
                        failed_m |= psm[h] & __builtin_amdgcn_ballot_w64(sk[h] != f0);
                    else   /* any sector per participant: k_front_sectors puts the tile's records in order */
                        __builtin_amdgcn_raw_buffer_store_b16((short)sk[h], bsk, ons[h] ? ((f / STEPS) * URF_TILE + tstar + np + urf_popc_below(psm[h])) * 2u : URF_OOB,
                                                              0, URF_FRONT_NT);
                    const unsigned so = (f / STEPS) * URF_TILE + tstar + np + urf_popc_below(psm[h]);
                    const unsigned o4 = ons[h] ? so * 4u : URF_OOB;
                    const float pr = urf_sqrt_rn_normal(rho2[h]);   /* star_shaped_search.cpp:164: sqrtf(x * x + y * y) */
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(pr), bsr, o4, 0, URF_FRONT_NT);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(Z[h]), bsz, o4, 0, URF_FRONT_NT);
                    __builtin_amdgcn_raw_buffer_store_b16((short)((stp * L + h * 64u + lane) | (on[h] ? 0u : URF_SLOT_OFF)), bss, ons[h] ? so * 2u : URF_OOB, 0,
                                                          URF_FRONT_NT);
                    np += (unsigned)__popcll(psm[h]);
                }
                if constexpr (!MS) {
#pragma unroll
                    for (unsigned q = 0; q < NK; q++) {
                        if (NK == 1u || stp / 64u == q) {   /* (uniform) */
                            stepkey_v[q] = lane == stp - q * 64u ? (int)f0 : stepkey_v[q];
                            stepcnt_v[q] = lane == stp - q * 64u ? (int)np : stepcnt_v[q];
                        }
                    }
                }
                tstar += np;
            }
#pragma unroll
            for (unsigned h = 0; h < NH; h++)
                troi += (unsigned)__popcll(roim[h]);
        }
        /* the lasers' windows move on by their new ring points; what has become decidable is decided */
#pragma unroll
        for (unsigned h = 0; h < NH; h++) {
            urf_front_ring<CP>& r = R[h];
            if (on[h]) {
                if (PH == 1u) {
                    const double s2 = (double)X[h] * (double)X[h] + (double)Y[h] * (double)Y[h];
                    r.maxs = s2 > r.maxs ? s2 : r.maxs;
                    r.pw |= 1u << (f & 31u);
                }
                r.econf = true;
                r.win.template push<PH>(Z[h], f - Fs);
            }
            if (PH == 0u)
                continue;
            /* (straight-line: every lane computes, the lanes without a new point are masked out at the end -- branches around the
             * tests put the four results through registers and selects) */
            const bool full = r.win.full();
            const bool c_in = r.win.c_in(on[h]), p_in = r.win.p_in(on[h]);
            const bool hz = r.win.hz(curbH), hx = r.win.hx(curbH);
            /* (lane masks combined as masks: `&` on bools mixed with the wave-uniform switches went through 0 / 1 integers in vector
             * registers -- v_cndmask, v_and, v_cmp per term) */
            bool zz = false, xz = false, ez = false, ex = false;
            /* a window that began inside this march (a block border with a hole in the halo, a ring that has just entered the
             * region of interest): positions unknown here, k_front_finish decides */
            if (use_z) {   /* (uniform) */
                zz = c_in && full && hz;
                if (!from_start)
                    ez = c_in && !full;
            }
            if (use_x) {
                xz = p_in && full && hx;
                if (!from_start)
                    ex = p_in && !full;
            }
            if (__ballot(zz | xz | ez | ex) != 0ull) {   /* (uniform) */
                urf_front_push(cbuf, ncb, zz | ez, (r.win.centre_firing() + Fs) * L + h * 64u + lane, zz ? URF_FC_ZZ : URF_FC_EDGE_Z);
                urf_front_push(cbuf, ncb, xz | ex, (r.win.marked_firing() + Fs) * L + h * 64u + lane, xz ? URF_FC_XZ : URF_FC_EDGE_X);
                if (ncb > URF_FRONT_CBUF - 128u)
                    urf_front_flush(a, s, cbuf, ncb, overflow);
            }
        }
    };
    /* the presence words of 32 firings (64 lasers: a tile; 128: two) */
    auto pres_end = [&](const unsigned pt) {
#pragma unroll
        for (unsigned h = 0; h < NH; h++) {
            if (mine)
                LAY::pres(a, s)[(size_t)pt * L + h * 64u + lane] = R[h].pw;
            R[h].pw = 0;
        }
    };
    auto tile_end = [&](const unsigned t) {
        const size_t row = (size_t)s * a.tiles + t;
        if (lane == 0)
            a.tile_roi[row] = troi;
        if constexpr (MS) {
            /* the tile's participants, where k_front_sectors finds them: it writes the whole row */
            if (lane == 0)
                a.tsoff[row * (K + 1) + K] = (uint16_t)tstar;
        } else if (STAR) {
            /* sector k starts with the first step whose sector is >= k (urf_split_holey's construction: the steps' keys with the empty
             * steps filled in from the left must not fall; bisection over them).  A register per 64 steps, the running values carried from
             * one to the next */
            unsigned fk[NK], sbase_q[NK];
            unsigned carry = 0, total = 0;
#pragma unroll
            for (unsigned q = 0; q < NK; q++) {
                const bool held = W == 64u || lane < W;   /* this lane holds a step */
                const unsigned k1 = (held && (unsigned)stepkey_v[q] != URF_SEC_NONE) ? (unsigned)stepkey_v[q] + 1u : 0u;
                unsigned m = urf_wave_scan_max(k1);
                m = m > carry ? m : carry;
                unsigned exc = (unsigned)__shfl_up((int)m, 1);
                exc = lane == 0 ? carry : exc;
                if (__ballot(k1 != 0u && k1 < exc) != 0ull)
                    failed = true;   /* (uniform) the sectors fall inside the tile (the sweep's seam, an unorganised cloud) */
                fk[q] = m;
                carry = (unsigned)__builtin_amdgcn_readlane((int)m, 63);
                const unsigned sc = held ? (unsigned)stepcnt_v[q] : 0u;
                const unsigned sinc = urf_wave_scan_add(sc) + total;
                sbase_q[q] = sinc - sc;   /* lane j: participating points of the steps in front of step q * 64 + j; W < 64: lane W holds the tile's total */
                total = (unsigned)__builtin_amdgcn_readlane((int)sinc, 63);
            }
            for (unsigned k0 = 0; k0 <= K; k0 += 64u) {
                const unsigned k = k0 + lane;
                unsigned cnt = 0;   /* number of steps whose filled-in key + 1 is < k + 1 (the keys do not fall: a count per register adds up) */
#pragma unroll
                for (unsigned q = 0; q < NK; q++) {
                    unsigned lo = 0;
#pragma unroll
                    for (unsigned st = W / 2u; st > 0; st >>= 1) {
                        const unsigned v = (unsigned)__shfl((int)fk[q], (int)(lo + st - 1u));
                        lo += v < k + 1u ? st : 0u;
                    }
                    const unsigned v = (unsigned)__shfl((int)fk[q], (int)lo);
                    lo += (lo == W - 1u && v < k + 1u) ? 1u : 0u;
                    cnt += lo;
                }
                unsigned so;
                if constexpr (W < 64u) {
                    so = (unsigned)__shfl((int)sbase_q[0], (int)cnt);   /* (lane W holds the tile's total) */
                } else {
                    so = total;
#pragma unroll
                    for (unsigned q = 0; q < NK; q++) {
                        const unsigned v = (unsigned)__shfl((int)sbase_q[q], (int)(cnt & 63u));
                        so = (cnt >> 6) == q ? v : so;
                    }
                }
                if (k <= K)
                    a.tsoff[row * (K + 1) + k] = (uint16_t)so;
            }
        }
        troi = 0;
        tstar = 0;
#pragma unroll
        for (unsigned q = 0; q < NK; q++) {
            stepkey_v[q] = (int)URF_SEC_NONE;
            stepcnt_v[q] = 0;
        }
    };

    /* The points arrive four firings ahead, in four register sets (of NH halves) that are refilled as soon as they have been used: no
     * copies between sets (a copy waits for its source), every wait is for a load issued three firings ago. */
    float px[4][NH], py[4][NH], pz[4][NH];
    auto ld = [&](const unsigned j, const unsigned f) {
#pragma unroll
        for (unsigned h = 0; h < NH; h++) {
            /* (a lane behind the scan's end, a lane without a laser: one point of the scan for all of them, never looked at) */
            const unsigned i = f * L + h * 64u + lane, o = i < mylen ? i : len - 1u;
            px[j][h] = gx[o];
            py[j][h] = gy[o];
            pz[j][h] = gz[o];
        }
    };
#pragma unroll
    for (unsigned j = 0; j < 4; j++)
        ld(j, Fs + j);
    for (unsigned f = Fs; f < F0; f += 4) {
#pragma unroll
        for (unsigned j = 0; j < 4; j++) {
            step(std::integral_constant<unsigned, 0u>{}, f + j, px[j], py[j], pz[j]);
            ld(j, f + j + 4u);
        }
    }
    auto give_back = [&]() {
        a.front_ok[s] = 0u;
        if (ok == URF_FRONT_ROWS)
            a.table_redo[s] = 1u;   /* (nobody has checked the rest of the scan against the rows' table) */
    };
    for (unsigned f = F0; f < F1; f += 4) {
#pragma unroll
        for (unsigned j = 0; j < 4; j++) {
            if (f + j < F1)   /* (uniform: the scan's last tile may end anywhere) */
                step(std::integral_constant<unsigned, 1u>{}, f + j, px[j], py[j], pz[j]);
            ld(j, f + j + 4u);
        }
        if (((f + 4u) & 31u) == 0u || f + 4u >= F1)   /* (uniform) */
            pres_end(f >> 5);
        if (((f + 4u) % STEPS) == 0u || f + 4u >= F1) {   /* (uniform) the tile is complete */
            tile_end(f / STEPS);
            if (failed_m != 0ull || __ballot(failed | overflow) != 0ull) {   /* (uniform) */
                give_back();
                return;
            }
        }
    }
    for (unsigned f = F1; f < Fe; f += 4) {
#pragma unroll
        for (unsigned j = 0; j < 4; j++) {
            if (f + j < Fe)
                step(std::integral_constant<unsigned, 2u>{}, f + j, px[j], py[j], pz[j]);
            ld(j, f + j + 4u);
        }
    }
#pragma unroll
    for (unsigned h = 0; h < NH; h++) {
        urf_front_ring<CP>& r = R[h];
        /* the block's last ring points of every laser: their windows reach behind the march */
        if (!to_end) {
            /* the CP newest, oldest first: none has been a centre, the CP - H newest have not been x_zero's marked point either */
            auto tail = [&](auto bk) {
                constexpr unsigned back = decltype(bk)::value;
                const bool in = r.win.in_block(back);
                const unsigned what = (use_z ? URF_FC_EDGE_Z : 0u) | ((use_x && back < CP - H) ? URF_FC_EDGE_X : 0u);
                if (ncb > URF_FRONT_CBUF - 64u)
                    urf_front_flush(a, s, cbuf, ncb, overflow);
                urf_front_push(cbuf, ncb, in && what != 0u, (r.win.firing(back) + Fs) * L + h * 64u + lane, what);
            };
            URF_FRONT_TAIL_CALLS(CP, tail)
        }
        LAY::maxs_of_block(a, s, b)[h * 64u + lane] = (unsigned long long)__double_as_longlong(r.maxs);
        /* one laser, one ring -- over the whole scan: the blocks agree through the scan's two tables */
        if (r.econf) {
            const unsigned o1 = atomicCAS(&LAY::lane_ring(a, s)[h * 64u + lane], 0xffffffffu, r.E);
            const unsigned o2 = atomicCAS(&a.front_ring_lane[(size_t)s * C + r.E], 0xffffffffu, h * 64u + lane);
            failed = failed | (o1 != 0xffffffffu && o1 != r.E) | (o2 != 0xffffffffu && o2 != h * 64u + lane);
        }
    }
    urf_front_flush(a, s, cbuf, ncb, overflow);
    if (failed_m != 0ull || __ballot(failed | overflow) != 0ull)
        give_back();
}

/* one kernel per laser count and per curbPoints, each under a name of its own (tools/kernel_resources.py lists kernels by their base
 * identifier) and with its own waves per SIMD.  The window is 2 * CP + 1 registers per laser.  64 / 32 / 16 lasers: 1..5 fit five waves per
 * SIMD, 6..8 (13, 15, 17 heights and a fourth / fifth register of firing numbers) get the next budget (four waves, 128 registers).  128
 * lasers, two windows and two sets of prefetched points: 1..7 hold three (168 registers; 7 fills them without a spill), 8 -- two windows of
 * 17 heights and 2 x 5 registers of firing numbers -- gets two (256 registers). */
#ifndef URF_FRONT_WAVES_WIDE
#define URF_FRONT_WAVES_WIDE 4
#endif
#ifndef URF_FRONT128_WAVES
#define URF_FRONT128_WAVES 3
#endif
#ifndef URF_FRONT128_WAVES_WIDE
#define URF_FRONT128_WAVES_WIDE 2
#endif
#define URF_FRONT_WAVES_OF(L, CP) \
    ((L) > 64u ? ((CP) <= 7 ? URF_FRONT128_WAVES : URF_FRONT128_WAVES_WIDE) : ((CP) <= 5 ? URF_FRONT_WAVES : URF_FRONT_WAVES_WIDE))
#define URF_FRONT_KERNEL(name, L, CP)                                                                                                         \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(URF_FRONT_WAVES_OF(L, CP), URF_FRONT_WAVES_OF(L, CP))))               \
    void name(urf_kargs a, urf_dev_params dp)                                                                                                 \
    {                                                                                                                                       \
        __shared__ urf_u2 cbuf[URF_FRONT_CBUF];                                                                                               \
        if (!dp.p.star_shaped_method)                                                                                                         \
            urf_front_body<false, false, L, CP>(a, dp, cbuf);                                                                                 \
        else if (!dp.p.starbeam_filter)                                                                                                       \
            urf_front_body<true, false, L, CP>(a, dp, cbuf);                                                                                  \
        else                                                                                                                                  \
            urf_front_body<true, true, L, CP>(a, dp, cbuf);                                                                                   \
    }
/* curbPoints 5 in every front mode (128 lasers: with urf_set_front_lasers128 on) ... */
URF_FRONT_KERNEL(k_front, 64u, 5)
URF_FRONT_KERNEL(k_front32, 32u, 5)
URF_FRONT_KERNEL(k_front16, 16u, 5)
URF_FRONT_KERNEL(k_front128, 128u, 5)
/* ... and 1..8 with urf_set_front_mode(ctx, 3) (64 lasers) and urf_set_front_curb_points(ctx, 1) (32, 16 and 128).  Nothing in the body counts
 * per wave what is counted per firing: the halos (HPRE, HPRE_WIDE, HPOST) are firings, and a laser meets at most one ring point per firing
 * whatever L is; fw[] holds firings relative to Fs (at most front_tpb * URF_TILE / 16 + 20 < 65536); candidate indices are (firing) * L +
 * laser slot.  The finish step is k_front_finish_cp* (k_front_finish128_cp*): it takes the laser count from its layout. */
#define URF_FRONT_CP_X(n) \
    URF_FRONT_KERNEL(k_front_cp##n, 64u, n) URF_FRONT_KERNEL(k_front32_cp##n, 32u, n) URF_FRONT_KERNEL(k_front16_cp##n, 16u, n) URF_FRONT_KERNEL(k_front128_cp##n, 128u, n)
URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X
/* ... and the multi-sector instances (urf_front_body's MS), the two bodies of the star-shaped search -- with the search off sectors do
 * not matter and the host launches the plain kernel.  The budgets of their plain siblings.  curbPoints 5 (urf_set_front_multi_sector) ... */
#define URF_FRONT_KERNEL_MS(name, L, CP)                                                                                                      \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(URF_FRONT_WAVES_OF(L, CP), URF_FRONT_WAVES_OF(L, CP))))               \
    void name(urf_kargs a, urf_dev_params dp)                                                                                                 \
    {                                                                                                                                       \
        __shared__ urf_u2 cbuf[URF_FRONT_CBUF];                                                                                               \
        if (!dp.p.starbeam_filter)                                                                                                            \
            urf_front_body<true, false, L, CP, true>(a, dp, cbuf);                                                                            \
        else                                                                                                                                  \
            urf_front_body<true, true, L, CP, true>(a, dp, cbuf);                                                                             \
    }
URF_FRONT_KERNEL_MS(k_front_ms, 64u, 5)
URF_FRONT_KERNEL_MS(k_front32_ms, 32u, 5)
URF_FRONT_KERNEL_MS(k_front16_ms, 16u, 5)
URF_FRONT_KERNEL_MS(k_front128_ms, 128u, 5)
/* ... and the others of 1..8 (urf_set_front_multi_sector_curb_points on top of it; which of them a call may take at all is the plain
 * instances' rule: urf_policy::curb_points_ok) */
#define URF_FRONT_CP_X(n)                                                                                                                     \
    URF_FRONT_KERNEL_MS(k_front_ms_cp##n, 64u, n) URF_FRONT_KERNEL_MS(k_front32_ms_cp##n, 32u, n) URF_FRONT_KERNEL_MS(k_front16_ms_cp##n, 16u, n) \
    URF_FRONT_KERNEL_MS(k_front128_ms_cp##n, 128u, n)
URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X

/* ------------------------------------------------------------------------- */
/* k_front_finish                                                              */
/* ------------------------------------------------------------------------- */
#define URF_FINISH_CHUNK 768u   /* candidates per chunk (each may be listed twice): 12 KB of LDS */
#ifndef URF_FINISH_THREADS
#define URF_FINISH_THREADS 256   /* four waves and <= 40 KB of LDS per scan: four workgroups per CU, a batch of 1024 scans in one round (A/B 256 / 512 /
                                    * 1024 threads: cfg3 0.186 / 0.184 / 0.206 ms, the reference's default region of interest 0.210 / 0.241 / 0.264) */
#endif
template <unsigned NL>   /* urf_front_lay::NL: 64 or 128 */
struct urf_finish_shared_t {
    unsigned n[NL];              /* ring points of laser slot l */
    unsigned ring[NL];           /* its ring (0xffffffff: the slot holds no ring point) */
    unsigned ncurb[NL];          /* curb points of ring r (channels <= NL) */
    int q[4];
    unsigned n_pend;             /* entries of the scan's list of points to mark */
    unsigned nx, nz;             /* x_zero / z_zero items of the chunk at hand */
    unsigned tot[NL > 64u ? 1 : 0];   /* ring points of the scan, where two waves add them up (up to 64 slots: a wave shuffle, and no word here) */
    unsigned qsum[URF_FINISH_THREADS / NL][NL];
};

/* firing of the ring point in front of / behind firing f in lane l; 0xffffffff: none */
/* (P: word (f >> 5) * L + l, L = 1 << lsh lasers per firing) */
__device__ __forceinline__ unsigned urf_front_prev(const unsigned* P, unsigned lsh, unsigned l, unsigned f)
{
    unsigned t = f >> 5;
    unsigned w = P[(t << lsh) + l] & ((1u << (f & 31u)) - 1u);
    while (w == 0u) {
        if (t == 0u)
            return 0xffffffffu;
        t--;
        w = P[(t << lsh) + l];
    }
    return t * 32u + 31u - (unsigned)__clz((int)w);
}
__device__ __forceinline__ unsigned urf_front_next(const unsigned* P, unsigned lsh, unsigned ntiles, unsigned l, unsigned f)
{
    unsigned t = f >> 5;
    unsigned w = (f & 31u) == 31u ? 0u : P[(t << lsh) + l] & ~((2u << (f & 31u)) - 1u);
    while (w == 0u) {
        t++;
        if (t >= ntiles)
            return 0xffffffffu;
        w = P[(t << lsh) + l];
    }
    return t * 32u + (unsigned)__ffs((int)w) - 1u;
}

/* part 0: everything.  Parts 1 and 2 (r6): what does not depend on the star-shaped search -- positions, ring sizes, the candidates of the
 * two detectors and their marks -- as a launch of its own on a SECOND stream, next to k_index / k_star_sort_* / k_star_walk (it waits for
 * scattered loads, they for vector issue: urf_api.hip), and the star-shaped hits, the lists' hand-over to k_beams and the overflow tables
 * behind the walk.  The counters travel from part 1 to part 2 through front_st.
 * CP = params.curbPoints (h = CP / 2): the ring positions both detectors accept and how far their neighbours lie, as in the march.  Nothing
 * else in here knows CP, and what knows the laser count asks the layout (urf_front_lay<W128>: k_front_finish*, k_front_finish128*).  The two
 * families differ in ONE piece of code besides: how the scan's ring points are added up (64 slots: a wave shuffle; 128: an LDS atomic). */
template <unsigned CP, bool W128>
__device__ __forceinline__ void urf_front_finish_body(urf_kargs a, urf_dev_params dp, unsigned part)
{
    using LAY = urf_front_lay<W128>;
    constexpr unsigned NL = LAY::NL;
    __shared__ urf_finish_shared_t<NL> S;
    extern __shared__ unsigned sh_finish[];   /* P[tiles][64] presence words | B[tiles][64] (u16) ring points of the lane in the tiles before (tiles: LAY::tiles) */
    constexpr unsigned H = CP / 2u;
    const unsigned tiles = LAY::tiles(a);
    const unsigned s = blockIdx.x, tid = threadIdx.x;
    const unsigned ok = a.front_ok[s];
    if (!ok)
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned ntiles = (len + URF_TILE - 1) / URF_TILE;
    /* L lasers per firing: candidate index = firing * L + laser slot (its place in the input), presence words per 32 firings and slot */
    const unsigned lsh = LAY::lsh(a), L = 1u << lsh, lm = L - 1u;
    const unsigned npt = (((len + lm) >> lsh) + 31u) >> 5;   /* (L = 64: ntiles; always npt * L <= tiles * 64) */
    const unsigned C = (unsigned)dp.p.channels, K = (unsigned)dp.p.sectors;
    const urf_scan_info in = a.info[s];
    if (in.status != URF_OK)
        return;
    unsigned* const P = sh_finish;
    uint16_t* const B = (uint16_t*)(sh_finish + tiles * 64u);
    urf_u2* const chunk = (urf_u2*)(sh_finish + tiles * 96u);   /* [2 * URF_FINISH_CHUNK] a chunk of the candidate list, by kind */
    unsigned* const st = LAY::st(a, s);   /* [0..NL) ncurb, then LAY::ST_*: part 1 -> part 2 */
    urf_u2* const pend = a.front_all + (size_t)s * a.front_cand_cap;   /* (index, flags) of what phase M has to mark; later the list of all curb points */
    const unsigned sb = urf_sbase(a, s);
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, ok, gx, gy, gz);
    auto passed = [&](unsigned idx, unsigned flag) {
        const unsigned e = atomicAdd(&S.n_pend, 1u);
        if (e < a.front_cand_cap)
            pend[e] = urf_u2{ idx, flag };
    };
    unsigned m_from = 0;   /* phase M starts here in the list */
    if (part != 2u) {
    const urf_u2* const cand = a.front_cand + (size_t)s * a.front_cand_cap;
    const unsigned nc_raw = a.front_ncand[s];
    const unsigned nc = nc_raw < a.front_cand_cap ? nc_raw : a.front_cand_cap;
    for (unsigned k = tid; k < npt * L; k += URF_FINISH_THREADS)
        P[k] = LAY::pres(a, s)[k];
    if (tid < NL) {
        S.ncurb[tid] = 0;
        S.ring[tid] = LAY::lane_ring(a, s)[tid];
    }
    if (tid == 0) {
        st[LAY::ST_RING10] = 0;
        if constexpr (W128)
            S.tot[0] = 0;
        S.q[0] = (int)urf_fbits(0.f);
        S.q[1] = (int)urf_fbits(180.f);
        S.q[2] = (int)urf_fbits(180.f);
        S.q[3] = (int)urf_fbits(360.f);
        S.n_pend = 0;
    }
    __syncthreads();
    /* positions: the tiles in as many stretches as the workgroup has waves, per lane; then the stretches' sums */
    {
        constexpr unsigned NP = URF_FINISH_THREADS / NL;
        const unsigned l = tid & (NL - 1u), prt = tid / NL;
        const unsigned nt = l < L ? npt : 0u;   /* (the slots from L on hold no laser) */
        const unsigned tq = (nt + NP - 1u) / NP, ta = prt * tq < nt ? prt * tq : nt, tb = ta + tq < nt ? ta + tq : nt;
        unsigned run = 0;
        for (unsigned t = ta; t < tb; t++)
            run += (unsigned)__popc(P[(t << lsh) + l]);
        S.qsum[prt][l] = run;
        __syncthreads();
        unsigned add = 0, all = 0;
        for (unsigned p = 0; p < NP; p++) {
            add += p < prt ? S.qsum[p][l] : 0u;
            all += S.qsum[p][l];
        }
        for (unsigned t = ta; t < tb; t++) {
            B[(t << lsh) + l] = (uint16_t)add;
            add += (unsigned)__popc(P[(t << lsh) + l]);
        }
        if (prt == 0)
            S.n[l] = all;
    }
    /* ring sizes, the scan's summary, the rings' largest ranges */
    if (tid < C)
        a.ring_cnt[(size_t)s * C + tid] = 0;
    __syncthreads();
    if (tid < NL) {
        const unsigned r = S.ring[tid], n = r != 0xffffffffu ? S.n[tid] : 0u;
        unsigned tot = n;   /* the scan's ring points: one wave holds every slot, or two waves add them up in LDS */
        if constexpr (!W128)
            for (int o = 32; o > 0; o >>= 1)
                tot += __shfl_xor(tot, o);
        if (r != 0xffffffffu) {
            if constexpr (W128)
                atomicAdd(&S.tot[0], n);
            a.ring_cnt[(size_t)s * C + r] = n;
            unsigned long long m = 0;
            const unsigned nblk = (ntiles + a.front_tpb - 1u) / a.front_tpb;
            for (unsigned b0 = 0; b0 < nblk; b0 += 8u) {   /* (eight blocks' values in flight: one after the other this lane's chain was sixteen round trips) */
                unsigned long long v[8];
#pragma unroll
                for (unsigned b = 0; b < 8; b++)
                    v[b] = LAY::maxs(a, s, b0 + b < nblk ? b0 + b : b0, tid);
#pragma unroll
                for (unsigned b = 0; b < 8; b++)
                    m = v[b] > m ? v[b] : m;
            }
            a.maxdist[(size_t)s * C + r] = (float)__builtin_sqrt(__longlong_as_double((long long)m));
            a.vis[(size_t)s * C + r] = urf_vis{ __builtin_inff(), -__builtin_inff() };
            if (r == 10u)
                st[LAY::ST_RING10] = n;
        }
        /* (the summary's two counts are written behind k_index -- below -- which may still find the scan below the 30-point threshold) */
        if constexpr (!W128)
            if (tid == 0)
                st[LAY::ST_RING_PTS] = tot;
    }
    if constexpr (W128) {
        __syncthreads();
        if (tid == 0)
            st[LAY::ST_RING_PTS] = S.tot[0];
    }
    /* The candidates.  One wave-instruction costs the same with one busy lane as with sixty-four, and every kind of candidate has
     * its own expensive chain (x_zero: three f64 roots and a division; z_zero: ten differences, two roots, a division; a passed
     * test: the reference's azimuth -- a root, a division, an arc sine).  A wave that met all kinds in one iteration ran all
     * chains with a few lanes each: 1 200 instructions per iteration, 0.18 ms per 1024 scans.  So the list is worked off in
     * chunks, a chunk PARTITIONED by kind in LDS, each kind by whole waves, what passed collected and marked by whole waves:
     *   phase X   x_zero items    (XZ, EDGE_X)
     *   phase Z   z_zero items    (ZZ, EDGE_Z)
     *   phase M   the points that got a mark, and the star-shaped hits: record flag, azimuth, ring list, quadrants.
     * An item makes ONE memory round trip for its data: neighbours' firings from the presence words in LDS, then the point, the
     * neighbours and x_zero's table values requested together. */
    constexpr unsigned CH = URF_FINISH_CHUNK;
    for (unsigned c0 = 0; c0 < nc; c0 += CH) {
        const unsigned cn = nc - c0 < CH ? nc - c0 : CH;
        if (tid == 0) {
            S.nx = 0;
            S.nz = 0;
        }
        __syncthreads();
        /* partition: x_zero items from the front, z_zero items from the back (an item of a block's end may be both) */
        for (unsigned e = tid; e < cn; e += URF_FINISH_THREADS) {
            const urf_u2 cd = cand[c0 + e];
            if (cd.y & (URF_FC_XZ | URF_FC_EDGE_X))
                chunk[atomicAdd(&S.nx, 1u)] = cd;
            if (cd.y & (URF_FC_ZZ | URF_FC_EDGE_Z))
                chunk[2u * CH - 1u - atomicAdd(&S.nz, 1u)] = cd;
        }
        __syncthreads();
        const unsigned nx = S.nx, nz = S.nz;
        /* phase X: x_zero_method.cpp:30-68 marks p = j + h for j = p - h in [curbPoints, n - 1 - curbPoints] */
        if (dp.p.x_zero_method)
            for (unsigned e = tid; e < nx; e += URF_FINISH_THREADS) {
                const urf_u2 cd = chunk[e];
                const unsigned idx = cd.x, l = idx & lm, f = idx >> lsh;
                const unsigned n = S.n[l];
                const unsigned p = (unsigned)B[((f >> 5) << lsh) + l] + (unsigned)__popc(P[((f >> 5) << lsh) + l] & ((1u << (f & 31u)) - 1u));
                if (!(p >= CP + H && p + (CP - H) < n))
                    continue;
                unsigned fj = f, f3 = f;
#pragma unroll
                for (unsigned k = 0; k < H; k++)
                    fj = urf_front_prev(P, lsh, l, fj);
#pragma unroll
                for (unsigned k = 0; k < CP - H; k++)
                    f3 = urf_front_next(P, lsh, npt, l, f3);
                const unsigned ij = (fj << lsh) + l, i3 = (f3 << lsh) + l;
                const float pz = gz[idx], xj = gx[ij], yj = gy[ij], zj = gz[ij], x3 = gx[i3], y3 = gy[i3], z3 = gz[i3];
                const float nyj = a.newY[p - H], ny2 = a.newY[p], ny3 = a.newY[p + (CP - H)];
                bool heights = true;
                if (cd.y & URF_FC_EDGE_X)   /* (the march has not looked at the heights) */
                    heights = (__builtin_fabsf(zj - pz) >= dp.p.curbHeight || __builtin_fabsf(z3 - pz) >= dp.p.curbHeight) &&
                              (double)__builtin_fabsf(zj - z3) >= 0.05;
                if (heights && urf_x_zero_angle_vals(nyj, ny2, ny3, dp.p.angleFilter1, dp.x_angle_thr, xj, yj, x3, y3, zj, pz, z3))
                    passed(idx, 2u);
            }
        /* phase Z: z_zero_method.cpp:21-72 for the centre p */
        if (dp.p.z_zero_method)
            for (unsigned e = tid; e < nz; e += URF_FINISH_THREADS) {
                const urf_u2 cd = chunk[2u * CH - 1u - e];
                const unsigned idx = cd.x, l = idx & lm, f = idx >> lsh;
                const unsigned n = S.n[l];
                const unsigned p = (unsigned)B[((f >> 5) << lsh) + l] + (unsigned)__popc(P[((f >> 5) << lsh) + l] & ((1u << (f & 31u)) - 1u));
                if (!(p >= CP && p + CP < n))
                    continue;
                unsigned im[CP], ip[CP];
                {
                    unsigned g = f;
#pragma unroll
                    for (unsigned k = 0; k < CP; k++) {
                        g = urf_front_prev(P, lsh, l, g);
                        im[k] = (g << lsh) + l;
                    }
                    g = f;
#pragma unroll
                    for (unsigned k = 0; k < CP; k++) {
                        g = urf_front_next(P, lsh, npt, l, g);
                        ip[k] = (g << lsh) + l;
                    }
                }
                const bool needz = (cd.y & URF_FC_EDGE_Z) != 0u;   /* (the march has not looked at the heights) */
                float xm[CP], ym[CP], zm[CP], xp[CP], yp[CP], zp[CP];
#pragma unroll
                for (unsigned k = 0; k < CP; k++)
                    zm[k] = zp[k] = 0.f;
                const float px = gx[idx], py = gy[idx], pz = gz[idx];
#pragma unroll
                for (unsigned k = 0; k < CP; k++) {
                    xm[k] = gx[im[k]];
                    ym[k] = gy[im[k]];
                    xp[k] = gx[ip[k]];
                    yp[k] = gy[ip[k]];
                }
                /* (what bounds this kernel is the rate at which a CU takes scattered 4-byte loads -- one cache line per lane and
                 * instruction: the heights are only asked for by a wave that holds such an item) */
                if (__ballot(needz) != 0ull) {
#pragma unroll
                    for (unsigned k = 0; k < CP; k++) {
                        zm[k] = gz[needz ? im[k] : idx];
                        zp[k] = gz[needz ? ip[k] : idx];
                    }
                }
                bool heights = true;
                if (needz) {
                    const float azp = __builtin_fabsf(pz);
                    float max1 = azp, max2 = azp;
#pragma unroll
                    for (unsigned k = 0; k < CP; k++) {
                        const float za = __builtin_fabsf(zm[k]), zb = __builtin_fabsf(zp[k]);
                        max1 = za > max1 ? za : max1;
                        max2 = zb > max2 ? zb : max2;
                    }
                    heights = (max1 - azp >= dp.p.curbHeight || max2 - azp >= dp.p.curbHeight) && (double)__builtin_fabsf(max1 - max2) >= 0.05;
                }
                if (heights) {
                    auto xy = [&](int pos, float& xx, float& yy) {   /* pos: ring position; the centre's is p */
                        const int rel = pos - (int)p;
                        xx = rel < 0 ? xm[-rel - 1] : xp[rel - 1];
                        yy = rel < 0 ? ym[-rel - 1] : yp[rel - 1];
                    };
                    if (urf_z_zero_angle(dp.inv_cp, dp.p.angleFilter2, dp.z_angle_thr, xy, (int)p, (int)CP, px, py))
                        passed(idx, 4u);
                }
            }
        __syncthreads();   /* the chunk's buffer is free for the next one */
    }
    } else {
        /* part 2: the counters of part 1 */
        if (tid < NL) {
            S.ncurb[tid] = st[tid];
            S.ring[tid] = LAY::lane_ring(a, s)[tid];
        }
        if (tid < 4)
            S.q[tid] = (int)st[LAY::ST_QUAD + tid];
        if (tid == 0)
            S.n_pend = st[LAY::ST_NPEND];
        m_from = st[LAY::ST_NPEND];
        __syncthreads();
    }
    /* lidar_segmentation.cpp:235-242: the star-shaped hits (the walk reported them as input indices; -1: none or on no ring) */
    if (part != 1u && dp.p.star_shaped_method)
        for (unsigned k = tid; k < K; k += URF_FINISH_THREADS) {
            const int h = a.star_hit[(size_t)s * K + k];
            if (h >= 0)
                passed((unsigned)h, 1u);
        }
    __syncthreads();
    /* phase M.  A ring point that has a detector's mark: its record's flag (whoever sets the first one lists the point), the
     * reference's azimuth, its ring's list, ring 1's quadrants (urf_ring_point: lidar_segmentation.cpp:245-269, blind_spots.cpp:
     * 19-56).  The atomic is on its way while the azimuth is worked out.  The list of all curb points (the rings whose own list
     * overflows) takes the places of the entries already read: entry e is rewritten by the thread that read it. */
    const unsigned n_pend = S.n_pend < a.front_cand_cap ? S.n_pend : a.front_cand_cap;
    for (unsigned e = m_from + tid; e < n_pend; e += URF_FINISH_THREADS) {
        const urf_u2 pd = pend[e];
        const unsigned idx = pd.x, r = S.ring[idx & lm];
        const float px = gx[idx], py = gy[idx];
        const unsigned old = atomicOr(&a.rec[sb + idx], pd.y << URF_REC_FLAG_SHIFT);
        float d2;
        const float az = urf_azimuth(px, py, &d2);
        urf_u2 out = urf_u2{ 0u, 0xffffffffu };   /* (ring 0xffffffff: not a list entry) */
        if (((old >> URF_REC_FLAG_SHIFT) & 7u) == 0u) {   /* otherwise: already a curb point, listed by whoever marked it first */
            const unsigned ec = atomicAdd(&S.ncurb[r], 1u);
            if (ec < URF_CURB_LIST)
                a.curb_az[((size_t)s * C + r) * URF_CURB_LIST + ec] = az;
            out = urf_u2{ __float_as_uint(az), r };
            if (r == 1u && dp.p.blind_spots) {
                const int ab = (int)urf_fbits(az);
                if (az >= 0.f && az < 90.f)
                    atomicMax(&S.q[0], ab);
                else if (az >= 90.f && az < 180.f)
                    atomicMin(&S.q[1], ab);
                else if (az >= 180.f && az < 270.f)
                    atomicMax(&S.q[2], ab);
                else if (az < 360.f)
                    atomicMin(&S.q[3], ab);
            }
        }
        pend[e] = out;
    }
    __syncthreads();
    if (part == 1u) {   /* (uniform) the counters for part 2 */
        if (tid < NL)
            st[tid] = S.ncurb[tid];
        if (tid < 4)
            st[LAY::ST_QUAD + tid] = (unsigned)S.q[tid];
        if (tid == 0)
            st[LAY::ST_NPEND] = n_pend;
        return;
    }
    /* the scan's summary (lidar_segmentation.cpp:605-608: road_probably = every point of sorted ring 10) */
    if (tid == 0) {
        a.info[s].n_ring_pts = st[LAY::ST_RING_PTS];
        a.info[s].n_ring10 = in.n_rings > 10 ? st[LAY::ST_RING10] : 0u;
    }
    /* what k_beams reads (k_ring's epilogue) */
    if (tid < 4 && dp.p.blind_spots && in.n_rings > 1)
        a.quad[(size_t)s * 4 + tid] = __uint_as_float((unsigned)S.q[tid]);
    for (unsigned r = tid; r < in.n_rings; r += URF_FINISH_THREADS)
        a.curb_cnt[(size_t)s * C + r] = S.ncurb[r] <= URF_CURB_LIST ? S.ncurb[r] : URF_CURB_DENSE;
    /* a ring with more curb points than its list holds (rough ground): the per-degree tables instead, from the scan's
     * list of all curb points -- sufmin[i] = smallest curb azimuth >= i, premax[i] = largest <= i, NaN = none.  (The presence
     * words are no longer needed: their memory holds the two tables of the ring at hand.) */
    const unsigned n_all = n_pend;
    int* const cmin = (int*)sh_finish;
    int* const cmax = cmin + URF_DEG_CELLS;
    for (unsigned r = 0; r < in.n_rings; r++) {
        if (S.ncurb[r] <= URF_CURB_LIST)
            continue;   /* (uniform) */
        __syncthreads();
        for (unsigned i = tid; i < URF_DEG_CELLS; i += URF_FINISH_THREADS) {
            cmin[i] = URF_INT_NONE_MIN;
            cmax[i] = -1;
        }
        __syncthreads();
        for (unsigned e = tid; e < n_all; e += URF_FINISH_THREADS) {
            const urf_u2 v = a.front_all[(size_t)s * a.front_cand_cap + e];
            if (v.y != r)
                continue;
            const float az = __uint_as_float(v.x);
            int cl = (int)__builtin_floorf(az), ch = (int)__builtin_ceilf(az);
            cl = cl < 0 ? 0 : (cl > 360 ? 360 : cl);
            ch = ch < 0 ? 0 : (ch > 360 ? 360 : ch);
            atomicMin(&cmin[cl], (int)v.x);
            atomicMax(&cmax[ch], (int)v.x);
        }
        __syncthreads();
        if (tid < 64) {   /* one wave: running maximum upwards, running minimum downwards */
            float* sm = a.sufmin + ((size_t)s * C + r) * URF_DEG_CELLS;
            float* pm = a.premax + ((size_t)s * C + r) * URF_DEG_CELLS;
            /* six cells per lane, one scan across the wave each way */
            unsigned up[6], dn[6];
#pragma unroll
            for (unsigned e = 0; e < 6; e++) {
                const unsigned i = 6u * tid + e;
                up[e] = i < URF_DEG_CELLS ? (unsigned)(cmax[i] + 1) : 0u;
                dn[e] = i < URF_DEG_CELLS ? ~(unsigned)cmin[URF_DEG_CELLS - 1 - i] : 0u;
                if (e) {
                    up[e] = up[e] > up[e - 1] ? up[e] : up[e - 1];
                    dn[e] = dn[e] > dn[e - 1] ? dn[e] : dn[e - 1];
                }
            }
            const unsigned iu = urf_wave_scan_max(up[5]), id = urf_wave_scan_max(dn[5]);
            unsigned pu = (unsigned)__shfl_up((int)iu, 1), pd = (unsigned)__shfl_up((int)id, 1);
            if (tid == 0)
                pu = pd = 0;
#pragma unroll
            for (unsigned e = 0; e < 6; e++) {
                const unsigned i = 6u * tid + e;
                if (i < URF_DEG_CELLS) {
                    const unsigned u = up[e] > pu ? up[e] : pu, d = dn[e] > pd ? dn[e] : pd;
                    pm[i] = u == 0 ? __builtin_nanf("") : __uint_as_float(u - 1u);
                    sm[URF_DEG_CELLS - 1 - i] = (d == 0x80000000u || d == 0u) ? __builtin_nanf("") : __uint_as_float(~d);
                }
            }
        }
    }
}
/* one kernel per family and per curbPoints, as for k_front (k_front_finish, k_front_finish128: 5; urf_set_front_curb_points: the others) */
#define URF_FRONT_FINISH_KERNEL(name, CP, W128)                                                               \
    __global__ __launch_bounds__(URF_FINISH_THREADS) void name(urf_kargs a, urf_dev_params dp, unsigned part) \
    {                                                                                                         \
        urf_front_finish_body<CP, W128>(a, dp, part);                                                         \
    }
URF_FRONT_FINISH_KERNEL(k_front_finish, 5u, false)
URF_FRONT_FINISH_KERNEL(k_front_finish128, 5u, true)
#define URF_FRONT_CP_X(n) URF_FRONT_FINISH_KERNEL(k_front_finish_cp##n, n, false) URF_FRONT_FINISH_KERNEL(k_front_finish128_cp##n, n, true)
URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X

/* ------------------------------------------------------------------------- */
/* k_label_front                                                               */
/* ------------------------------------------------------------------------- */
/* k_label for a scan of the fused front end: the records are in input order, eight consecutive points per thread,
 * the label bytes leave as one 8-byte store.  Same decisions as k_label (urf_road_test on the record's quantised
 * azimuth, the exact azimuth where that leaves a decision open). */
__global__ __launch_bounds__(URF_LABEL_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_label_front(urf_kargs a, urf_dev_params dp)
{
    using LAY = urf_front_lay<false>;
    __shared__ unsigned cnt_road, cnt_curb, n_unsure;
    __shared__ unsigned un_idx[URF_LABEL_UNSURE], un_ring[URF_LABEL_UNSURE];
    __shared__ __attribute__((aligned(8))) uint8_t lab_t[LAY::NL * (URF_TILE / LAY::NL + 8u)];   /* (row-major scans) [laser][firings of the tile + 8]: 64 x 40, 32 x 72, 16 x 136 */
    unsigned s = blockIdx.y, t = blockIdx.x;
    {   /* the tiles of one scan on one XCD (k_label: the scan's window table is fetched by one L2) */
        const unsigned T = gridDim.x, lin = blockIdx.y * T + blockIdx.x;
        const unsigned grp = lin / (8u * T), r = lin - grp * (8u * T);
        if ((grp + 1u) * 8u <= gridDim.y) {
            s = grp * 8u + (r & 7u);
            t = r >> 3;
        }
    }
    const unsigned tid = threadIdx.x;
    const unsigned ok = a.front_ok[s];
    if (!ok)
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned tbase = t * URF_TILE;
    if (tbase >= len)
        return;
    const bool rows = ok == URF_FRONT_ROWS;   /* (uniform) the labels go where the points came from: row l, column f */
    const unsigned lsh = a.front_lsh, wsh = 11u - lsh;   /* L = 1 << lsh lasers per firing, 1 << wsh firings per tile */
    const unsigned F = len >> lsh;
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, ok, gx, gy, gz);
    const unsigned C = (unsigned)dp.p.channels;
    const size_t row = (size_t)s * a.tiles + t;
    const unsigned sb = urf_sbase(a, s);
    const urf_scan_info in = a.info[s];
    const unsigned troi = a.tile_roi[row];
    const unsigned i0 = tbase + tid * 8u;   /* this thread's eight points: one eighth of a firing */
    /* (the firings behind the scan's last one were never visited: their words hold whatever an earlier call left) */
    const unsigned in_scan = i0 + 8u <= len ? 0xffu : (i0 < len ? (1u << (len - i0)) - 1u : 0u);
    const unsigned bits = ((const uint8_t*)(a.roi_bits + row * URF_FRONT_STEPS))[tid] & in_scan;
    uint8_t* const out = a.labels + off + i0;
    const bool whole = tbase + URF_TILE <= len && ((uintptr_t)(a.labels + off + tbase) & 7u) == 0;   /* (uniform) */
    /* row-major: the tile's firings x lasers through LDS, then 8 columns of a row per thread */
    auto store_rows = [&](const unsigned (&lb)[8]) {
        const unsigned RS = (1u << wsh) + 8u;
        const unsigned stp = (tid * 8u) >> lsh, l0 = (tid * 8u) & ((1u << lsh) - 1u);
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
            lab_t[(l0 + e) * RS + stp] = (uint8_t)lb[e];
        __syncthreads();
        const unsigned l = tid >> (wsh - 3u), c0 = (tid & ((1u << (wsh - 3u)) - 1u)) * 8u, f0 = (t << wsh) + c0;
        uint8_t* const o = a.labels + off + (size_t)l * F + f0;
        const uint8_t* const src = &lab_t[l * RS + c0];
        if (f0 + 8u <= F && ((uintptr_t)o & 7u) == 0) {
            *(uint2*)o = *(const uint2*)src;
        } else {
            for (unsigned e = 0; e < 8; e++)
                if (f0 + e < F)
                    o[e] = src[e];
        }
    };
    if (in.status != URF_OK || troi == 0) {
        if (rows) {
            const unsigned zero[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
            store_rows(zero);
        } else if (whole) {
            *(uint2*)out = make_uint2(0u, 0u);
        } else {
            for (unsigned e = 0; e < 8; e++)
                if (i0 + e < len)
                    out[e] = 0;
        }
        return;
    }
    if (tid == 0) {
        cnt_road = 0;
        cnt_curb = 0;
        n_unsure = 0;
    }
    __syncthreads();
    const urf_win* win = a.win + (size_t)s * C * URF_DEG_CELLS;
    unsigned rec[8];
    if (bits) {   /* (the records of a firing without a point in the region of interest were never written) */
        const uint4 r0 = *(const uint4*)(a.rec + sb + i0), r1 = *(const uint4*)(a.rec + sb + i0 + 4);
        rec[0] = r0.x; rec[1] = r0.y; rec[2] = r0.z; rec[3] = r0.w;
        rec[4] = r1.x; rec[5] = r1.y; rec[6] = r1.z; rec[7] = r1.w;
    } else {
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
            rec[e] = LAY::RING_NONE;
    }
    unsigned lab[8];
    unsigned my_road = 0, my_curb = 0;
    /* (four points at a time: the window ends of four are requested before any of them is looked at) */
#pragma unroll
    for (unsigned h = 0; h < 8; h += 4) {
    float whi[4], wlo[4];
#pragma unroll
    for (unsigned q = 0; q < 4; q++) {
        const unsigned e = h + q;
        const bool on = ((bits >> e) & 1u) && (rec[e] & LAY::RING_MASK) != LAY::RING_NONE;
        const unsigned c = on ? (rec[e] & LAY::RING_MASK) : 0u;
        const float az = urf_az_decode(rec[e] >> URF_REC_AZ_SHIFT);
        const bool num = az == az;
        int cf = num ? (int)__builtin_floorf(az) : 0, cb = num ? (int)__builtin_ceilf(az) : 0;
        cf = cf < 0 ? 0 : (cf > 360 ? 360 : cf);
        cb = cb < 0 ? 0 : (cb > 360 ? 360 : cb);
        whi[q] = win[c * URF_DEG_CELLS + cf].hi;
        wlo[q] = win[c * URF_DEG_CELLS + cb].lo;
    }
#pragma unroll
    for (unsigned q = 0; q < 4; q++) {
        const unsigned e = h + q;
        const bool roi = (bits >> e) & 1u;
        const bool on = roi && (rec[e] & LAY::RING_MASK) != LAY::RING_NONE;
        const unsigned c = rec[e] & LAY::RING_MASK;
        const bool curb = on && ((rec[e] >> URF_REC_FLAG_SHIFT) & 7u) != 0;
        const float az = urf_az_decode(rec[e] >> URF_REC_AZ_SHIFT), eps = urf_fast_az_eps(az) + URF_REC_AZ_QERR;
        const float fl = __builtin_floorf(az);
        bool road = az <= whi[q] || az >= wlo[q];
        const bool unsure = az < 0.0f || az - fl <= eps || (fl + 1.0f) - az <= eps || __builtin_fabsf(az - whi[q]) <= eps ||
                            __builtin_fabsf(az - wlo[q]) <= eps;
        /* (the label first, with a point whose decision is open as "not road"; THEN the branch for such a point: the lane masks above
         * are dead by then -- they used to live across it, and the compiler parked fourteen scalar registers per point in a vector
         * register's lanes, v_writelane by v_writelane) */
        const bool uns = unsure && on && !curb;
        road = road && on && !curb && !uns;
        lab[e] = !roi ? 0u
                      : (URF_FLAG_ROI | (on ? URF_FLAG_RING | (c == 10 ? URF_FLAG_RING10 : 0) | (curb ? URF_LABEL_CURB : 0) | (road ? URF_LABEL_ROAD : 0) : 0u));
        my_curb += curb ? 1u : 0u;
        my_road += road ? 1u : 0u;
        if (uns) {
            const unsigned u = atomicAdd(&n_unsure, 1u);
            if (u < URF_LABEL_UNSURE) {
                un_idx[u] = i0 + e;
                un_ring[u] = c;   /* corrected below */
            } else {   /* list full (pathological input) */
                float d2;
                bool dummy;
                const float xaz = urf_azimuth(gx[i0 + e], gy[i0 + e], &d2);
                if (urf_road_test(win + c * URF_DEG_CELLS, xaz, 0.0f, dummy)) {
                    lab[e] |= URF_LABEL_ROAD;
                    my_road++;
                }
            }
        }
    }
    }
    if (rows) {
        store_rows(lab);
    } else if (whole) {
        *(uint2*)out = make_uint2(lab[0] | lab[1] << 8 | lab[2] << 16 | lab[3] << 24, lab[4] | lab[5] << 8 | lab[6] << 16 | lab[7] << 24);
    } else {
        for (unsigned e = 0; e < 8; e++)
            if (i0 + e < len)
                out[e] = (uint8_t)lab[e];
    }
    __syncthreads();   /* the tile's stores come first, the corrections second */
    const unsigned nu = n_unsure < URF_LABEL_UNSURE ? n_unsure : URF_LABEL_UNSURE;
    if (tid < nu) {
        const unsigned i = un_idx[tid], c = un_ring[tid];
        bool dummy;
        float d2;
        const float az = urf_azimuth(gx[i], gy[i], &d2);
        if (urf_road_test(win + c * URF_DEG_CELLS, az, 0.0f, dummy)) {
            a.labels[off + (rows ? (size_t)(i & ((1u << lsh) - 1u)) * F + (i >> lsh) : (size_t)i)] = URF_FLAG_ROI | URF_FLAG_RING | (c == 10 ? URF_FLAG_RING10 : 0) | URF_LABEL_ROAD;
            my_road++;
        }
    }
    if (my_road)
        atomicAdd(&cnt_road, my_road);
    if (my_curb)
        atomicAdd(&cnt_curb, my_curb);
    __syncthreads();
    if (tid == 0) {
        urf_scan_info* o = &a.info[s];
        if (cnt_road)
            atomicAdd(&o->n_road, cnt_road);
        if (cnt_curb)
            atomicAdd(&o->n_curb, cnt_curb);
    }
}

/* k_label_front for the records of k_front128: the ring in eight bits (urf_front_lay<true>::RING_*), 128 rows of 16 + 8 label bytes for a
 * row-major tile.  A COPY of the kernel above, and kept as one on purpose: as urf_label_front_body<W128> behind two wrappers both kernels
 * came out with 58 registers instead of 52 and their event bracket 1 - 2.6 % longer (profiles/front_one_finish.md) -- the text was the same,
 * the wrapper alone changes what the compiler makes of it.  What differs: lsh (a constant), the record's ring mask and "none", lab_t's shape. */
__global__ __launch_bounds__(URF_LABEL_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_label_front128(urf_kargs a, urf_dev_params dp)
{
    using LAY = urf_front_lay<true>;
    __shared__ unsigned cnt_road, cnt_curb, n_unsure;
    __shared__ unsigned un_idx[URF_LABEL_UNSURE], un_ring[URF_LABEL_UNSURE];
    __shared__ __attribute__((aligned(8))) uint8_t lab_t[LAY::NL * (URF_TILE / LAY::NL + 8u)];   /* (row-major scans) [laser][firings of the tile + 8] */
    unsigned s = blockIdx.y, t = blockIdx.x;
    {   /* the tiles of one scan on one XCD (k_label: the scan's window table is fetched by one L2) */
        const unsigned T = gridDim.x, lin = blockIdx.y * T + blockIdx.x;
        const unsigned grp = lin / (8u * T), r = lin - grp * (8u * T);
        if ((grp + 1u) * 8u <= gridDim.y) {
            s = grp * 8u + (r & 7u);
            t = r >> 3;
        }
    }
    const unsigned tid = threadIdx.x;
    const unsigned ok = a.front_ok[s];
    if (!ok)
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned tbase = t * URF_TILE;
    if (tbase >= len)
        return;
    const bool rows = ok == URF_FRONT_ROWS;   /* (uniform) the labels go where the points came from: row l, column f */
    constexpr unsigned lsh = URF_FRONT128_LSH, wsh = 11u - lsh;   /* L = 1 << lsh lasers per firing, 1 << wsh firings per tile */
    const unsigned F = len >> lsh;
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, ok, gx, gy, gz);
    const unsigned C = (unsigned)dp.p.channels;
    const size_t row = (size_t)s * a.tiles + t;
    const unsigned sb = urf_sbase(a, s);
    const urf_scan_info in = a.info[s];
    const unsigned troi = a.tile_roi[row];
    const unsigned i0 = tbase + tid * 8u;   /* this thread's eight points: one eighth of a firing */
    /* (the firings behind the scan's last one were never visited: their words hold whatever an earlier call left) */
    const unsigned in_scan = i0 + 8u <= len ? 0xffu : (i0 < len ? (1u << (len - i0)) - 1u : 0u);
    const unsigned bits = ((const uint8_t*)(a.roi_bits + row * URF_FRONT_STEPS))[tid] & in_scan;
    uint8_t* const out = a.labels + off + i0;
    const bool whole = tbase + URF_TILE <= len && ((uintptr_t)(a.labels + off + tbase) & 7u) == 0;   /* (uniform) */
    /* row-major: the tile's firings x lasers through LDS, then 8 columns of a row per thread */
    auto store_rows = [&](const unsigned (&lb)[8]) {
        const unsigned RS = (1u << wsh) + 8u;
        const unsigned stp = (tid * 8u) >> lsh, l0 = (tid * 8u) & ((1u << lsh) - 1u);
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
            lab_t[(l0 + e) * RS + stp] = (uint8_t)lb[e];
        __syncthreads();
        const unsigned l = tid >> (wsh - 3u), c0 = (tid & ((1u << (wsh - 3u)) - 1u)) * 8u, f0 = (t << wsh) + c0;
        uint8_t* const o = a.labels + off + (size_t)l * F + f0;
        const uint8_t* const src = &lab_t[l * RS + c0];
        if (f0 + 8u <= F && ((uintptr_t)o & 7u) == 0) {
            *(uint2*)o = *(const uint2*)src;
        } else {
            for (unsigned e = 0; e < 8; e++)
                if (f0 + e < F)
                    o[e] = src[e];
        }
    };
    if (in.status != URF_OK || troi == 0) {
        if (rows) {
            const unsigned zero[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
            store_rows(zero);
        } else if (whole) {
            *(uint2*)out = make_uint2(0u, 0u);
        } else {
            for (unsigned e = 0; e < 8; e++)
                if (i0 + e < len)
                    out[e] = 0;
        }
        return;
    }
    if (tid == 0) {
        cnt_road = 0;
        cnt_curb = 0;
        n_unsure = 0;
    }
    __syncthreads();
    const urf_win* win = a.win + (size_t)s * C * URF_DEG_CELLS;
    unsigned rec[8];
    if (bits) {   /* (the records of a firing without a point in the region of interest were never written) */
        const uint4 r0 = *(const uint4*)(a.rec + sb + i0), r1 = *(const uint4*)(a.rec + sb + i0 + 4);
        rec[0] = r0.x; rec[1] = r0.y; rec[2] = r0.z; rec[3] = r0.w;
        rec[4] = r1.x; rec[5] = r1.y; rec[6] = r1.z; rec[7] = r1.w;
    } else {
#pragma unroll
        for (unsigned e = 0; e < 8; e++)
            rec[e] = LAY::RING_NONE;
    }
    unsigned lab[8];
    unsigned my_road = 0, my_curb = 0;
    /* (four points at a time: the window ends of four are requested before any of them is looked at) */
#pragma unroll
    for (unsigned h = 0; h < 8; h += 4) {
    float whi[4], wlo[4];
#pragma unroll
    for (unsigned q = 0; q < 4; q++) {
        const unsigned e = h + q;
        const bool on = ((bits >> e) & 1u) && (rec[e] & LAY::RING_MASK) != LAY::RING_NONE;
        const unsigned c = on ? (rec[e] & LAY::RING_MASK) : 0u;
        const float az = urf_az_decode(rec[e] >> URF_REC_AZ_SHIFT);
        const bool num = az == az;
        int cf = num ? (int)__builtin_floorf(az) : 0, cb = num ? (int)__builtin_ceilf(az) : 0;
        cf = cf < 0 ? 0 : (cf > 360 ? 360 : cf);
        cb = cb < 0 ? 0 : (cb > 360 ? 360 : cb);
        whi[q] = win[c * URF_DEG_CELLS + cf].hi;
        wlo[q] = win[c * URF_DEG_CELLS + cb].lo;
    }
#pragma unroll
    for (unsigned q = 0; q < 4; q++) {
        const unsigned e = h + q;
        const bool roi = (bits >> e) & 1u;
        const bool on = roi && (rec[e] & LAY::RING_MASK) != LAY::RING_NONE;
        const unsigned c = rec[e] & LAY::RING_MASK;
        const bool curb = on && ((rec[e] >> URF_REC_FLAG_SHIFT) & 7u) != 0;
        const float az = urf_az_decode(rec[e] >> URF_REC_AZ_SHIFT), eps = urf_fast_az_eps(az) + URF_REC_AZ_QERR;
        const float fl = __builtin_floorf(az);
        bool road = az <= whi[q] || az >= wlo[q];
        const bool unsure = az < 0.0f || az - fl <= eps || (fl + 1.0f) - az <= eps || __builtin_fabsf(az - whi[q]) <= eps ||
                            __builtin_fabsf(az - wlo[q]) <= eps;
        /* (the label first, with a point whose decision is open as "not road"; THEN the branch for such a point: the lane masks above
         * are dead by then -- they used to live across it, and the compiler parked fourteen scalar registers per point in a vector
         * register's lanes, v_writelane by v_writelane) */
        const bool uns = unsure && on && !curb;
        road = road && on && !curb && !uns;
        lab[e] = !roi ? 0u
                      : (URF_FLAG_ROI | (on ? URF_FLAG_RING | (c == 10 ? URF_FLAG_RING10 : 0) | (curb ? URF_LABEL_CURB : 0) | (road ? URF_LABEL_ROAD : 0) : 0u));
        my_curb += curb ? 1u : 0u;
        my_road += road ? 1u : 0u;
        if (uns) {
            const unsigned u = atomicAdd(&n_unsure, 1u);
            if (u < URF_LABEL_UNSURE) {
                un_idx[u] = i0 + e;
                un_ring[u] = c;   /* corrected below */
            } else {   /* list full (pathological input) */
                float d2;
                bool dummy;
                const float xaz = urf_azimuth(gx[i0 + e], gy[i0 + e], &d2);
                if (urf_road_test(win + c * URF_DEG_CELLS, xaz, 0.0f, dummy)) {
                    lab[e] |= URF_LABEL_ROAD;
                    my_road++;
                }
            }
        }
    }
    }
    if (rows) {
        store_rows(lab);
    } else if (whole) {
        *(uint2*)out = make_uint2(lab[0] | lab[1] << 8 | lab[2] << 16 | lab[3] << 24, lab[4] | lab[5] << 8 | lab[6] << 16 | lab[7] << 24);
    } else {
        for (unsigned e = 0; e < 8; e++)
            if (i0 + e < len)
                out[e] = (uint8_t)lab[e];
    }
    __syncthreads();   /* the tile's stores come first, the corrections second */
    const unsigned nu = n_unsure < URF_LABEL_UNSURE ? n_unsure : URF_LABEL_UNSURE;
    if (tid < nu) {
        const unsigned i = un_idx[tid], c = un_ring[tid];
        bool dummy;
        float d2;
        const float az = urf_azimuth(gx[i], gy[i], &d2);
        if (urf_road_test(win + c * URF_DEG_CELLS, az, 0.0f, dummy)) {
            a.labels[off + (rows ? (size_t)(i & ((1u << lsh) - 1u)) * F + (i >> lsh) : (size_t)i)] = URF_FLAG_ROI | URF_FLAG_RING | (c == 10 ? URF_FLAG_RING10 : 0) | URF_LABEL_ROAD;
            my_road++;
        }
    }
    if (my_road)
        atomicAdd(&cnt_road, my_road);
    if (my_curb)
        atomicAdd(&cnt_curb, my_curb);
    __syncthreads();
    if (tid == 0) {
        urf_scan_info* o = &a.info[s];
        if (cnt_road)
            atomicAdd(&o->n_road, cnt_road);
        if (cnt_curb)
            atomicAdd(&o->n_curb, cnt_curb);
    }
}

#endif /* URF_FRONT_HPP */
