/*
 * urf_k_front_explain.hpp -- k_front_explain: which rules of the fused front end's march (urf_front.hpp) a scan of the LAST call breaks,
 * counted for urf_front_explain (urf_api.hip).  Off the hot path: launched by that entry point and, in a context that turned
 * urf_set_front_auto on, behind the few calls that carry its learning pass (urf_k_front_digest.hpp); no other classify call knows it.
 *
 * It reads the call's points again and the scan's FINAL ring table (a.angle, info[s].n_rings) -- never the march's windows or its own
 * tables (front_lane_ring, front_ring_lane, the candidate lists), which a call without the fused kernels does not even fill -- and
 * decides per point what the march decides: region of interest, the ring by the reference's exact sequence (urf_exact_keys_body), the star
 * sector and whether the point takes part in the star-shaped search (beam filter included).  From those:
 *   one laser slot, one ring / one ring, one laser slot   two per-scan tables, claimed with atomicCAS as the march's block end claims its
 *                                                         own; a slot (a ring) that meets a second ring (slot) gets its bit in a per-scan
 *                                                         mask -- whichever block comes first, the same bits: the host counts them
 *   ring points on the sensor's axis (x == y == 0)        counted
 *   participants outside urf_sqrt_rn_normal's interval    counted
 *   firings whose participants lie in several sectors     counted, with the largest number of sectors in one firing
 *   tiles in which a participant's sector is smaller      counted (tile-local: the march's stepkeys and bisection are per tile)
 *   than an earlier participant's
 *
 * Grid (tiles, scans), one wave per block; lane = laser slot (two per lane at 128 lasers), the wave walks its tile's firings.  layout 0:
 * point f * L + l; layout 1, row-major: point l * F + f (strided loads: nobody waits for this kernel).  No LDS, no scratch memory.
 */
#ifndef URF_K_FRONT_EXPLAIN_HPP
#define URF_K_FRONT_EXPLAIN_HPP

#include "urf_kernels.hpp"

/* the per-scan record, 32-bit words (zeroed by the host before the launch) */
#define URF_FX_LANE_RING 0u     /* [128] ring + 1 of laser slot l (0: none yet) */
#define URF_FX_RING_LANE 128u   /* [128] laser slot + 1 of ring r */
#define URF_FX_LANE_MASK 256u   /* [4] bit l: slot l met a second ring */
#define URF_FX_RING_MASK 260u   /* [4] bit r: ring r was fed by a second slot */
#define URF_FX_AXIS 264u
#define URF_FX_RANGE 265u
#define URF_FX_MULTI 266u       /* firings with more than one sector */
#define URF_FX_MAX_SECTORS 267u
#define URF_FX_FALL 268u        /* tiles in which the sectors fall */
#define URF_FX_WORDS 272u

/* The per-scan rule: what a scan's record, its flag (front_ok), its candidate count, its status and its length say under the call's
 * settings -- `fused`, the URF_WHY_SCAN_* bits and the URF_ADVICE_* they ask for.  One function for the host's loop (urf_front_explain)
 * and for the device (k_front_digest, urf_k_front_digest.hpp).  The call's part: */
struct urf_fx_call {
    uint32_t front, front_rows, cand_cap;   /* a.front, a.front_rows, a.front_cand_cap */
    uint32_t rows;        /* the layout the record was counted in: 1 row-major */
    uint32_t lasers;      /* params.channels where it is 16, 32, 64 or 128, else 0 (no laser slots to speak of) */
    uint32_t ms;          /* the march was, or would have been, the multi-sector one (urf_policy::ms_ok) */
    uint32_t cp_other;    /* curbPoints != 5 */
    uint32_t call_why;    /* URF_WHY_CALL_* of the call as planned */
    uint32_t len;         /* a sweep of the callback path: the caller's number of points; 0: the scan's own length */
};
struct urf_fx_scan {
    uint32_t fused, scan, advice;
};
__host__ __device__ inline uint32_t urf_fx_bits4(const uint32_t* m)
{
    uint32_t n = 0;
    for (int k = 0; k < 4; k++)
        for (uint32_t v = m[k]; v; v &= v - 1u)
            n++;
    return n;
}
__host__ __device__ inline urf_fx_scan urf_front_scan_rule(const urf_fx_call& k, const uint32_t* r, uint32_t ok, uint32_t ncand, int status, uint32_t len)
{
    urf_fx_scan o = { (k.front && ok) ? 1u : 0u, 0u, 0u };
    if (status != URF_OK || len == 0u)
        return o;   /* URF_TOO_FEW_POINTS, an empty scan, a voided sweep: no rule applies */
    uint32_t scan = (urf_fx_bits4(r + URF_FX_LANE_MASK) ? URF_WHY_SCAN_LANE_TWO_RINGS : 0u) | (urf_fx_bits4(r + URF_FX_RING_MASK) ? URF_WHY_SCAN_RING_TWO_LANES : 0u) |
                    (r[URF_FX_AXIS] ? URF_WHY_SCAN_AXIS : 0u) | (r[URF_FX_RANGE] ? URF_WHY_SCAN_RANGE : 0u);
    if (k.rows && k.lasers && len % k.lasers != 0u)
        scan |= URF_WHY_SCAN_ROWS_LENGTH;
    if (scan)
        o.advice |= URF_ADVICE_NEVER;
    if (!k.ms) {
        const uint32_t ms = (r[URF_FX_MULTI] ? URF_WHY_SCAN_MULTI_SECTOR : 0u) | (r[URF_FX_FALL] ? URF_WHY_SCAN_SECTORS_FALL : 0u);
        if (ms)
            o.advice |= URF_ADVICE_MULTI_SECTOR | (k.cp_other ? URF_ADVICE_MULTI_SECTOR_CP : 0u);
        scan |= ms;
    }
    if (k.front && ncand > k.cand_cap)
        scan |= URF_WHY_SCAN_CANDIDATES, o.advice |= URF_ADVICE_CAPACITY;
    if (k.rows && k.front_rows == 0u)
        scan |= URF_WHY_SCAN_ROWS_SIGHTING, o.advice |= URF_ADVICE_CALL_AGAIN;
    if (!o.fused && !k.call_why && !scan)
        scan = URF_WHY_SCAN_OTHER, o.advice |= URF_ADVICE_CALL_AGAIN;
    o.scan = scan;
    return o;
}

__global__ __launch_bounds__(64) void k_front_explain(urf_kargs a, urf_dev_params dp, unsigned layout, uint32_t* __restrict__ recs)
{
    const unsigned s = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    if (len == 0u || a.info[s].status != URF_OK)
        return;   /* (uniform) an empty scan, URF_TOO_FEW_POINTS: no rule applies */
    const unsigned L = (unsigned)dp.p.channels;   /* (the host launches for 16, 32, 64 and 128 only) */
    const unsigned STEPS = URF_TILE / L;
    const bool rows = layout != 0u;
    if (rows && len % L != 0u)
        return;   /* (uniform) not `channels` whole rows: the host says so */
    const unsigned F = len / L;                              /* row-major: the rows' length */
    const unsigned nf = rows ? F : (len + L - 1u) / L;       /* firings of the scan */
    const unsigned f_first = t * STEPS;
    if (f_first >= nf)
        return;
    const unsigned f_end = f_first + STEPS < nf ? f_first + STEPS : nf;
    uint32_t* const rec = recs + (size_t)s * URF_FX_WORDS;
    const float* const tab = a.angle + (size_t)s * dp.p.channels;
    const unsigned nR = a.info[s].n_rings < L ? a.info[s].n_rings : L;   /* (a table holds at most `channels` entries) */
    const unsigned K = dp.p.star_shaped_method ? (unsigned)dp.p.sectors : 0u;
    const bool beam = dp.p.starbeam_filter != 0;
    const float* const gx = a.x + off;
    const float* const gy = a.y + off;
    const float* const gz = a.z + off;
    const unsigned NH = L > 64u ? 2u : 1u;

    unsigned seen[2] = { 0u, 0u };   /* ring + 1 this lane's slot has claimed or checked last (indexed by constants: registers) */
    unsigned n_axis = 0, n_range = 0, n_multi = 0, max_sec = 0;   /* (wave-uniform) */
    unsigned tile_max = 0;           /* largest sector + 1 among the tile's participants so far */
    bool fall = false;
    for (unsigned f = f_first; f < f_end; f++) {
        unsigned sk[2] = { URF_SEC_NONE, URF_SEC_NONE };
        unsigned long long pm[2] = { 0ull, 0ull };
#pragma unroll
        for (unsigned h = 0; h < 2u; h++) {
            if (h >= NH)
                continue;   /* (uniform) */
            const unsigned l = h * 64u + lane;
            const unsigned i = rows ? l * F + f : f * L + l;
            const bool valid = l < L && i < len;
            const unsigned o = valid ? i : 0u;
            const float x = gx[o], y = gy[o], z = gz[o];
            const bool roi = valid && urf_in_roi(dp.p, x, y, z);
            bool on = false, part = false;
            unsigned ring = URF_RING_NONE;
            if (roi) {
                /* (the body, inlined: a second caller of the shared urf_exact_keys changes k_split's register allocation) */
                const urf_exact_key ek = urf_exact_keys_body(tab, nR, dp.p.interval, x, y, z, K, dp.Kfi);
                ring = ek.ring;
                on = ring != URF_RING_NONE;
                unsigned k = ek.sector;
                if (K && beam && !urf_in_beam(a.beams[k], x, y))
                    k = URF_SEC_NONE;
                part = K != 0u && k != URF_SEC_NONE;
                sk[h] = part ? k : URF_SEC_NONE;
            }
            if (on && seen[h] != ring + 1u) {
                seen[h] = ring + 1u;
                const unsigned o1 = atomicCAS(&rec[URF_FX_LANE_RING + l], 0u, ring + 1u);
                if (o1 != 0u && o1 != ring + 1u)
                    atomicOr(&rec[URF_FX_LANE_MASK + (l >> 5)], 1u << (l & 31u));
                const unsigned o2 = atomicCAS(&rec[URF_FX_RING_LANE + ring], 0u, l + 1u);
                if (o2 != 0u && o2 != l + 1u)
                    atomicOr(&rec[URF_FX_RING_MASK + (ring >> 5)], 1u << (ring & 31u));
            }
            const float rho2 = x * x + y * y;
            n_axis += (unsigned)__popcll(__ballot(on && x == 0.0f && y == 0.0f));
            n_range += (unsigned)__popcll(__ballot(part && !(rho2 >= 0x1p-90f && rho2 <= 0x1p126f)));
            pm[h] = __ballot(part);
            /* the sectors fall: a participant's is smaller than one in front of it in the tile -- in an earlier firing or half (tile_max),
             * or in a lower lane of this one */
            const unsigned k1 = part ? sk[h] + 1u : 0u;
            const unsigned inc = urf_wave_scan_max(k1);
            unsigned exc = (unsigned)__shfl_up((int)inc, 1);
            exc = lane == 0u ? 0u : exc;
            exc = exc > tile_max ? exc : tile_max;
            fall = fall | (__ballot(part && k1 < exc) != 0ull);
            const unsigned hm = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
            tile_max = hm > tile_max ? hm : tile_max;
        }
        /* the firing's sectors: one round per distinct value (a sensor's firing: one to four) */
        unsigned ns = 0;
        while ((pm[0] | pm[1]) != 0ull) {   /* (uniform) */
            const unsigned key = pm[0] ? (unsigned)__builtin_amdgcn_readlane((int)sk[0], (int)((unsigned)__ffsll((long long)pm[0]) - 1u))
                                       : (unsigned)__builtin_amdgcn_readlane((int)sk[1], (int)((unsigned)__ffsll((long long)pm[1]) - 1u));
            pm[0] &= ~__ballot(sk[0] == key);
            pm[1] &= ~__ballot(sk[1] == key);
            ns++;
        }
        n_multi += ns > 1u ? 1u : 0u;
        max_sec = ns > max_sec ? ns : max_sec;
    }
    if (lane == 0u) {
        if (n_axis)
            atomicAdd(&rec[URF_FX_AXIS], n_axis);
        if (n_range)
            atomicAdd(&rec[URF_FX_RANGE], n_range);
        if (n_multi)
            atomicAdd(&rec[URF_FX_MULTI], n_multi);
        if (max_sec)
            atomicMax(&rec[URF_FX_MAX_SECTORS], max_sec);
        if (fall)
            atomicAdd(&rec[URF_FX_FALL], 1u);
    }
}

#endif /* URF_K_FRONT_EXPLAIN_HPP */
