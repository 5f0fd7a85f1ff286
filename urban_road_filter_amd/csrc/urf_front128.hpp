/*
 * urf_front128.hpp -- the fused front end (urf_front.hpp) for sweeps of 128 lasers per firing (urf_set_front_lasers128): firing order
 * (point f * 128 + l) or row-major (128 rows).  This header holds the march, the one kernel of the family with a body of its own:
 *
 *   k_front128          ONE wave per block, TWO lasers per lane: lane j marches lasers j and j + 64 (half 0 and half 1 of a firing), with
 *                       two windows (urf_front_window, urf_front.hpp) and two sets of per-ring state.  The two halves of a firing are
 *                       worked off back to back inside one step, so that everything that crosses lanes -- the slot rank of a star
 *                       participant, the one-sector test, the step's key and count -- spans the 128 lasers in input order with two
 *                       ballots and no LDS traffic or barrier, and the candidate buffer stays "the workgroup is the wave".  The price is
 *                       registers.  k_front128_cp{1,2,3,4,6,7,8} are the same body, urf_front128_body, for the
 *                       other curbPoints (urf_set_front_mode(ctx, 3) with urf_set_front_lasers128 and urf_set_front_curb_points on).
 *
 * The kernels around it -- k_front_finish128 (and _cp*), k_transpose128 (urf_front.hpp), k_rows_probe128 (urf_k_table.hpp) -- are the W128
 * instances of the bodies they share with 64 / 32 / 16 lasers, each a named wrapper next to its body; what is different about 128 lasers
 * there (the arrays, their strides, the record's ring in eight bits; the constants URF_FRONT128_L, _LSH, _TILES2, _ST_WORDS, _RING_*) is
 * written down once, in urf_front_lay<true> (urf_front.hpp).  k_label_front128 stands next to k_label_front there, as a kernel of its own.
 *
 * What they leave behind keeps the layout its readers know, indexed by f * 128 + l: region-of-interest bits (two 64-bit words per
 * firing), slots (stp * 128 + l < 2048), tsoff, candidate indices.  What was sized for 64 lanes has a sibling sized for 128
 * (urf_kargs::*128), allocated when the switch is turned on.  A tile is 16 firings and a presence word 32 of them: word
 * (f >> 5) * 128 + l covers two tiles, so the words per scan are counted for an even number of tiles (URF_FRONT128_TILES2), and a
 * block of the march holds an even number of tiles (front_tpb, urf_api.hip) -- no presence word is shared between two blocks.
 */
#ifndef URF_FRONT128_HPP
#define URF_FRONT128_HPP

#define URF_FRONT128_STEPS (URF_TILE / URF_FRONT128_L)   /* firings per tile: 16 */
/* Entries per scan of the candidate lists of these kernels.  The points that pass the march's height tests are counted per LASER, not per
 * column: a ring that crosses a curb hands on up to eleven centres (z_zero) and six marked points (x_zero) per crossing, a street has four
 * crossings per ring -- 128 x 68 = 8 704 for 128 lasers however short the sweep is (a 128 x 256 street of urf_synth_cloud: 5 200 - 5 600),
 * above the context's max(max_points / 8, 4096) for sweeps below 128 x 544.  Twice that for range noise; a list that overflows still only
 * hands its scan back.
 * curbPoints 1..8 (urf_set_front_curb_points): 2 * CP + 1 centres and CP + 1 marked points per crossing, at 8 that is 17 and 9 -- 4 x 26 = 104 per
 * laser: 128 x 104 = 13 312 here, below the cap as it is; 32 x 104 = 3 328 and 16 x 104 = 1 664 at 32 and 16 lasers, below the context's floor of
 * 4096 (a block's border adds at most 2 * CP edge items per laser: 16 more per block).  No cap grows for the new instances. */
#define URF_FRONT128_CAND_CAP(max_points) ((max_points) / 8u > 16384u ? (max_points) / 8u : 16384u)
#ifndef URF_FRONT128_WAVES
#define URF_FRONT128_WAVES 3           /* 168 registers: two windows, two sets of prefetched points */
#endif

/* what the march keeps per laser */
template <unsigned CP>
struct urf_front128_ring {
    unsigned E;          /* the table entry this laser's points are expected on */
    bool econf;          /* ... and a point of this march has confirmed it */
    urf_front_thr th;
    urf_front_window<CP> win;   /* its last 2 * CP + 1 ring points (urf_front.hpp) */
    double maxs;
    unsigned pw;
};

/* The march of urf_front_body (urf_front.hpp) for 128 lasers and curbPoints CP of 1..8: h = 0, 1 is the half of the firing, laser
 * h * 64 + lane.  Every array of two below is indexed by constants only (the loops over h are unrolled): registers. */
template <bool STAR, bool BEAM, unsigned CP>
__device__ __forceinline__ void urf_front128_body(const urf_kargs& a, const urf_dev_params& dp, urf_u2* cbuf)
{
    const unsigned s = blockIdx.y, b = blockIdx.x, lane = threadIdx.x;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned TPB = a.front_tpb;   /* (even: urf_api.hip) */
    const unsigned t_first = b * TPB;
    if (t_first * URF_TILE >= len)
        return;
    const unsigned ok = a.front_ok[s];
    if (ok == 0u)
        return;
    constexpr unsigned L = URF_FRONT128_L, C = L, STEPS = URF_FRONT128_STEPS;
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
    const unsigned tiles2 = URF_FRONT128_TILES2(a.tiles);
    const float *gx, *gy, *gz;
    urf_front_src(a, s, off, ok, gx, gy, gz);
    const __amdgpu_buffer_rsrc_t brec = urf_buf(a.rec + sb, len * 4u);
    const __amdgpu_buffer_rsrc_t bsr = urf_buf(a.sr + sb, a.tiles * URF_TILE * 4u), bsz = urf_buf(a.sz + sb, a.tiles * URF_TILE * 4u);
    const __amdgpu_buffer_rsrc_t bss = urf_buf(a.sslot + sb, a.tiles * URF_TILE * 2u);
    const unsigned nR = a.info[s].n_rings;
    const unsigned upto_v = a.table_upto[s];
    const unsigned upto = ok == URF_FRONT_ROWS ? 0u : (nR < C ? upto_v : 0xffffffffu);
    const float* const tab = a.angle + (size_t)s * dp.p.channels;
    const float curbH = dp.p.curbHeight;
    const bool use_x = dp.p.x_zero_method != 0, use_z = dp.p.z_zero_method != 0;

    urf_front128_ring<CP> R[2];
#pragma unroll
    for (unsigned h = 0; h < 2; h++) {
        R[h].E = h * 64u + lane;
        R[h].econf = false;
        R[h].th = urf_front_load_thr(a, s, C, R[h].E, nR);
        R[h].win.clear();
        R[h].maxs = 0.0;
        R[h].pw = 0u;
    }
    bool failed = false, overflow = false;
    unsigned long long failed_m = 0;   /* what the hot path finds wrong, as lane masks (wave-uniform) */
    unsigned ncb = 0;                  /* candidates in the wave's buffer */
    /* per tile (wave-uniform) */
    unsigned troi = 0, tstar = 0;
    int stepkey_v = (int)URF_SEC_NONE, stepcnt_v = 0;   /* lane j < 16: sector / participating points of step j of the tile */

    /* one firing.  PH 0: the halo in front of the block (windows fill), 1: the block, 2: the halo behind it (windows complete) */
    auto step = [&](auto ph, const unsigned f, const float (&X)[2], const float (&Y)[2], const float (&Z)[2]) {
        constexpr unsigned PH = decltype(ph)::value;
        const unsigned stp = f % STEPS;
        bool roi[2], on[2];
        unsigned long long roim[2];
#pragma unroll
        for (unsigned h = 0; h < 2; h++) {
            roi[h] = f * L + h * 64u + lane < len && urf_in_roi(dp.p, X[h], Y[h], Z[h]);
            roim[h] = __ballot(roi[h]);
        }
        if (PH == 1u && lane < 2u)   /* bit i of the scan's words: input point i */
            a.roi_bits[((size_t)s * a.tiles + f / STEPS) * (URF_TILE / 64u) + stp * 2u + lane] = lane ? roim[1] : roim[0];
        if ((roim[0] | roim[1]) == 0ull)
            return;   /* (uniform) nothing of this firing lies in the region of interest */
        float rho2[2], fi[2];
        unsigned sk[2];
        bool ons[2];
        unsigned long long psm[2] = { 0ull, 0ull };
#pragma unroll
        for (unsigned h = 0; h < 2; h++) {
            urf_front128_ring<CP>& r = R[h];
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
            if (PH == 1u) {
                /* the record, input order: ring (eight bits) | azimuth code */
                const unsigned azc_v = urf_az_code(urf_fast_azimuth_of(fi[h]));
                const unsigned azc = urf_fast_az_ok(x, y) ? azc_v : URF_REC_AZ_UNKNOWN;
                __builtin_amdgcn_raw_buffer_store_b32((azc << URF_REC_AZ_SHIFT) | (on[h] ? r.E : URF_FRONT128_RING_NONE), brec, i * 4u, 0, URF_FRONT_NT);
                if (STAR) {
                    if (BEAM && roi[h] && !urf_in_beam(a.beams[fs < 0 ? 0 : fs], x, y))
                        sk[h] = URF_SEC_NONE;
                    psm[h] = roim[h] & __builtin_amdgcn_ballot_w64(sk[h] != URF_SEC_NONE) & __builtin_amdgcn_ballot_w64((int)sk[h] >= 0);
                    ons[h] = roi[h] && sk[h] != URF_SEC_NONE && (int)sk[h] >= 0;
                    failed_m |= psm[h] & ~(__builtin_amdgcn_ballot_w64(rho2[h] >= 0x1p-90f) & __builtin_amdgcn_ballot_w64(rho2[h] <= 0x1p126f));
                }
            }
        }
        if (PH == 1u) {
            if (STAR) {
                /* star-shaped search: the firing's participants -- of BOTH halves -- share one sector, and their copies follow each
                 * other in input order: half 0's, then half 1's */
                unsigned f0 = URF_SEC_NONE;
                if (psm[0])
                    f0 = (unsigned)__builtin_amdgcn_readlane((int)sk[0], (int)((unsigned)__ffsll((long long)psm[0]) - 1u));
                else if (psm[1])
                    f0 = (unsigned)__builtin_amdgcn_readlane((int)sk[1], (int)((unsigned)__ffsll((long long)psm[1]) - 1u));
                const unsigned n0 = (unsigned)__popcll(psm[0]), n1 = (unsigned)__popcll(psm[1]);
#pragma unroll
                for (unsigned h = 0; h < 2; h++) {
                    failed_m |= psm[h] & __builtin_amdgcn_ballot_w64(sk[h] != f0);
                    const unsigned so = (f / STEPS) * URF_TILE + tstar + (h ? n0 : 0u) + urf_popc_below(psm[h]);
                    const unsigned o4 = ons[h] ? so * 4u : URF_OOB;
                    const float pr = urf_sqrt_rn_normal(rho2[h]);   /* star_shaped_search.cpp:164: sqrtf(x * x + y * y) */
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(pr), bsr, o4, 0, URF_FRONT_NT);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(Z[h]), bsz, o4, 0, URF_FRONT_NT);
                    __builtin_amdgcn_raw_buffer_store_b16((short)((stp * L + h * 64u + lane) | (on[h] ? 0u : URF_SLOT_OFF)), bss, ons[h] ? so * 2u : URF_OOB, 0,
                                                          URF_FRONT_NT);
                }
                stepkey_v = lane == stp ? (int)f0 : stepkey_v;
                stepcnt_v = lane == stp ? (int)(n0 + n1) : stepcnt_v;
                tstar += n0 + n1;
            }
            troi += (unsigned)__popcll(roim[0]) + (unsigned)__popcll(roim[1]);
        }
        /* the lasers' windows move on by their new ring points; what has become decidable is decided */
#pragma unroll
        for (unsigned h = 0; h < 2; h++) {
            urf_front128_ring<CP>& r = R[h];
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
            const bool full = r.win.full();
            const bool c_in = r.win.c_in(on[h]), p_in = r.win.p_in(on[h]);
            const bool hz = r.win.hz(curbH), hx = r.win.hx(curbH);
            bool zz = false, xz = false, ez = false, ex = false;
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
    /* the presence words of 32 firings (two tiles) */
    auto pres_end = [&](const unsigned pt) {
#pragma unroll
        for (unsigned h = 0; h < 2; h++) {
            a.front_pres128[(size_t)s * tiles2 * 64u + (size_t)pt * L + h * 64u + lane] = R[h].pw;
            R[h].pw = 0;
        }
    };
    auto tile_end = [&](const unsigned t) {
        const size_t row = (size_t)s * a.tiles + t;
        if (lane == 0)
            a.tile_roi[row] = troi;
        if (STAR) {
            /* sector k starts with the first step whose sector is >= k (urf_front_body's construction, bisection over the 16 steps) */
            const unsigned k1 = (lane < STEPS && (unsigned)stepkey_v != URF_SEC_NONE) ? (unsigned)stepkey_v + 1u : 0u;
            const unsigned fk = urf_wave_scan_max(k1);
            unsigned exc = (unsigned)__shfl_up((int)fk, 1);
            exc = lane == 0 ? 0u : exc;
            if (__ballot(k1 != 0u && k1 < exc) != 0ull)
                failed = true;   /* (uniform) the sectors fall inside the tile (the sweep's seam, an unorganised cloud) */
            const unsigned sc = lane < STEPS ? (unsigned)stepcnt_v : 0u;
            const unsigned sinc = urf_wave_scan_add(sc);
            const unsigned sbase_l = sinc - sc;   /* lane j: participating points of the steps in front of step j; lane 16: all */
            for (unsigned k0 = 0; k0 <= K; k0 += 64u) {
                const unsigned k = k0 + lane;
                unsigned lo = 0;   /* number of steps whose filled-in key + 1 is < k + 1 */
#pragma unroll
                for (unsigned st = STEPS / 2; st > 0; st >>= 1) {
                    const unsigned v = (unsigned)__shfl((int)fk, (int)(lo + st - 1u));
                    lo += v < k + 1u ? st : 0u;
                }
                {
                    const unsigned v = (unsigned)__shfl((int)fk, (int)lo);
                    lo += (lo == STEPS - 1u && v < k + 1u) ? 1u : 0u;
                }
                const unsigned so = (unsigned)__shfl((int)sbase_l, (int)lo);   /* (lane 16 holds the tile's total) */
                if (k <= K)
                    a.tsoff[row * (K + 1) + k] = (uint16_t)so;
            }
        }
        troi = 0;
        tstar = 0;
        stepkey_v = (int)URF_SEC_NONE;
        stepcnt_v = 0;
    };

    /* The points arrive four firings ahead, in four register sets (of two halves) that are refilled as soon as they have been used */
    float px[4][2], py[4][2], pz[4][2];
    auto ld = [&](const unsigned j, const unsigned f) {
#pragma unroll
        for (unsigned h = 0; h < 2; h++) {
            const unsigned i = f * L + h * 64u + lane, o = i < len ? i : len - 1u;   /* (behind the scan's end: one point of the scan, never looked at) */
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
    for (unsigned h = 0; h < 2; h++) {
        urf_front128_ring<CP>& r = R[h];
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
        a.front_maxs128[(size_t)s * tiles2 * 64u + (size_t)b * L + h * 64u + lane] = (unsigned long long)__double_as_longlong(r.maxs);
        /* one laser, one ring -- over the whole scan: the blocks agree through the scan's two tables */
        if (r.econf) {
            const unsigned o1 = atomicCAS(&a.front_lane_ring128[(size_t)s * L + h * 64u + lane], 0xffffffffu, r.E);
            const unsigned o2 = atomicCAS(&a.front_ring_lane[(size_t)s * C + r.E], 0xffffffffu, h * 64u + lane);
            failed = failed | (o1 != 0xffffffffu && o1 != r.E) | (o2 != 0xffffffffu && o2 != h * 64u + lane);
        }
    }
    urf_front_flush(a, s, cbuf, ncb, overflow);
    if (failed_m != 0ull || __ballot(failed | overflow) != 0ull)
        give_back();
}

/* one kernel per curbPoints (k_front128: 5).  Waves per SIMD: 1..7 hold three (168 registers; 7 fills them without a spill), 8 -- two
 * windows of 17 heights and 2 x 5 registers of firing numbers -- gets two (256 registers) */
#ifndef URF_FRONT128_WAVES_WIDE
#define URF_FRONT128_WAVES_WIDE 2
#endif
#define URF_FRONT128_WAVES_OF(CP) ((CP) <= 7 ? URF_FRONT128_WAVES : URF_FRONT128_WAVES_WIDE)
#define URF_FRONT128_KERNEL(name, CP)                                                                                                 \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(URF_FRONT128_WAVES_OF(CP), URF_FRONT128_WAVES_OF(CP))))       \
    void name(urf_kargs a, urf_dev_params dp)                                                                                         \
    {                                                                                                                                 \
        __shared__ urf_u2 cbuf[URF_FRONT_CBUF];                                                                                       \
        if (!dp.p.star_shaped_method)                                                                                                 \
            urf_front128_body<false, false, CP>(a, dp, cbuf);                                                                         \
        else if (!dp.p.starbeam_filter)                                                                                               \
            urf_front128_body<true, false, CP>(a, dp, cbuf);                                                                          \
        else                                                                                                                          \
            urf_front128_body<true, true, CP>(a, dp, cbuf);                                                                           \
    }
URF_FRONT128_KERNEL(k_front128, 5)
#define URF_FRONT_CP_X(n) URF_FRONT128_KERNEL(k_front128_cp##n, n)
URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X


#endif /* URF_FRONT128_HPP */
