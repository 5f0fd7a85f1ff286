/*
 * urf_front128_finish.hpp -- k_front_finish and k_label_front (urf_front.hpp) for 128 lasers per firing (curbPoints 5; the others of 1..8: k_front_finish128_cp*): the same
 * phases and the same arithmetic, with 128 rings' sizes, positions, largest ranges and curb lists, the 128-laser siblings of the
 * arrays that are sized for 64 lanes (urf_kargs::*128) and the record's ring in eight bits.  Included by urf_front128.hpp.
 */
#ifndef URF_FRONT128_FINISH_HPP
#define URF_FRONT128_FINISH_HPP

struct urf_finish128_shared {
    unsigned n[URF_FRONT128_L];       /* ring points of laser slot l */
    unsigned ring[URF_FRONT128_L];    /* its ring (0xffffffff: the slot holds no ring point) */
    unsigned ncurb[URF_FRONT128_L];   /* curb points of ring r */
    int q[4];
    unsigned n_pend;             /* entries of the scan's list of points to mark */
    unsigned nx, nz;             /* x_zero / z_zero items of the chunk at hand */
    unsigned tot;                /* ring points of the scan */
    unsigned qsum[URF_FINISH_THREADS / URF_FRONT128_L][URF_FRONT128_L];
};

/* parts as in urf_front_finish_body.  Dynamic LDS: P[tiles2][64] presence words | B[tiles2][64] (u16) | a chunk of the candidate list
 * (tiles2 = the scan's tiles rounded up to an even number: a presence word covers two tiles).
 * CP = params.curbPoints (k_front_finish128: 5, the default; k_front_finish128_cp*: the others of 1..8), H = CP / 2: the ring positions both
 * detectors accept and how far their neighbours lie, as in urf_front_finish_body.  Nothing else in here knows CP, and nothing that uses
 * it knows the laser count. */
template <unsigned CP = 5u>
__device__ __forceinline__ void urf_front128_finish_body(urf_kargs a, urf_dev_params dp, unsigned part)
{
    __shared__ urf_finish128_shared S;
    extern __shared__ unsigned sh_finish[];   /* P[tiles][64] presence words | B[tiles][64] (u16) ring points of the lane in the tiles before */
    constexpr unsigned H = CP / 2u;
    const unsigned tiles2 = URF_FRONT128_TILES2(a.tiles);
    const unsigned s = blockIdx.x, tid = threadIdx.x;
    const unsigned ok = a.front_ok[s];
    if (!ok)
        return;
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    const unsigned ntiles = (len + URF_TILE - 1) / URF_TILE;
    /* L lasers per firing: candidate index = firing * L + laser slot (its place in the input), presence words per 32 firings and slot */
    constexpr unsigned lsh = URF_FRONT128_LSH, L = URF_FRONT128_L, lm = L - 1u;
    const unsigned npt = (((len + lm) >> lsh) + 31u) >> 5;   /* (32 firings: two tiles; npt * L <= tiles2 * 64) */
    const unsigned C = (unsigned)dp.p.channels, K = (unsigned)dp.p.sectors;
    const urf_scan_info in = a.info[s];
    if (in.status != URF_OK)
        return;
    unsigned* const P = sh_finish;
    uint16_t* const B = (uint16_t*)(sh_finish + tiles2 * 64u);
    urf_u2* const chunk = (urf_u2*)(sh_finish + tiles2 * 96u);   /* [2 * URF_FINISH_CHUNK] a chunk of the candidate list, by kind */
    unsigned* const st = a.front_st128 + (size_t)s * URF_FRONT128_ST_WORDS;   /* [0..127] ncurb, [128..131] quadrants, [132] list length, [133] ring points, [134] ring 10's: part 1 -> part 2 */
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
        P[k] = a.front_pres128[(size_t)s * tiles2 * 64u + k];
    if (tid < L) {
        S.ncurb[tid] = 0;
        S.ring[tid] = a.front_lane_ring128[(size_t)s * L + tid];
    }
    if (tid == 0) {
        st[134] = 0;
        S.tot = 0;
        S.q[0] = (int)urf_fbits(0.f);
        S.q[1] = (int)urf_fbits(180.f);
        S.q[2] = (int)urf_fbits(180.f);
        S.q[3] = (int)urf_fbits(360.f);
        S.n_pend = 0;
    }
    __syncthreads();
    /* positions: the tiles in as many stretches as the workgroup has waves, per lane; then the stretches' sums */
    {
        constexpr unsigned NP = URF_FINISH_THREADS / L;
        const unsigned l = tid & lm, prt = tid >> lsh;
        const unsigned nt = npt;
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
    if (tid < L) {
        const unsigned r = S.ring[tid], n = r != 0xffffffffu ? S.n[tid] : 0u;
        if (r != 0xffffffffu) {
            atomicAdd(&S.tot, n);
            a.ring_cnt[(size_t)s * C + r] = n;
            unsigned long long m = 0;
            const unsigned nblk = (ntiles + a.front_tpb - 1u) / a.front_tpb;
            for (unsigned b0 = 0; b0 < nblk; b0 += 8u) {   /* (eight blocks' values in flight: one after the other this lane's chain was sixteen round trips) */
                unsigned long long v[8];
#pragma unroll
                for (unsigned b = 0; b < 8; b++)
                    v[b] = a.front_maxs128[(size_t)s * tiles2 * 64u + (size_t)(b0 + b < nblk ? b0 + b : b0) * L + tid];
#pragma unroll
                for (unsigned b = 0; b < 8; b++)
                    m = v[b] > m ? v[b] : m;
            }
            a.maxdist[(size_t)s * C + r] = (float)__builtin_sqrt(__longlong_as_double((long long)m));
            a.vis[(size_t)s * C + r] = urf_vis{ __builtin_inff(), -__builtin_inff() };
            if (r == 10u)
                st[134] = n;
        }
    }
    __syncthreads();
    if (tid == 0)
        st[133] = S.tot;   /* (the summary's two counts are written behind k_index -- below -- which may still find the scan below the 30-point threshold) */
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
        if (tid < L) {
            S.ncurb[tid] = st[tid];
            S.ring[tid] = a.front_lane_ring128[(size_t)s * L + tid];
        }
        if (tid < 4)
            S.q[tid] = (int)st[128u + tid];
        if (tid == 0)
            S.n_pend = st[132];
        m_from = st[132];
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
        if (tid < L)
            st[tid] = S.ncurb[tid];
        if (tid < 4)
            st[128u + tid] = (unsigned)S.q[tid];
        if (tid == 0)
            st[132] = n_pend;
        return;
    }
    /* the scan's summary (lidar_segmentation.cpp:605-608: road_probably = every point of sorted ring 10) */
    if (tid == 0) {
        a.info[s].n_ring_pts = st[133];
        a.info[s].n_ring10 = in.n_rings > 10 ? st[134] : 0u;
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
__global__ __launch_bounds__(URF_FINISH_THREADS) void k_front_finish128(urf_kargs a, urf_dev_params dp, unsigned part)
{
    urf_front128_finish_body(a, dp, part);
}
/* one kernel per curbPoints, as k_front_finish_cp* (urf_set_front_curb_points) */
#define URF_FRONT128_FINISH_KERNEL(name, CP)                                                                  \
    __global__ __launch_bounds__(URF_FINISH_THREADS) void name(urf_kargs a, urf_dev_params dp, unsigned part) \
    {                                                                                                         \
        urf_front128_finish_body<CP>(a, dp, part);                                                            \
    }
#define URF_FRONT_CP_X(n) URF_FRONT128_FINISH_KERNEL(k_front_finish128_cp##n, n)
URF_FRONT_CP_OTHERS(URF_FRONT_CP_X)
#undef URF_FRONT_CP_X

/* k_label_front (urf_front.hpp) for the records of k_front128: the ring in eight bits, 128 rows of 16 + 8 label bytes for a row-major tile. */
__global__ __launch_bounds__(URF_LABEL_TILE_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_label_front128(urf_kargs a, urf_dev_params dp)
{
    __shared__ unsigned cnt_road, cnt_curb, n_unsure;
    __shared__ unsigned un_idx[URF_LABEL_UNSURE], un_ring[URF_LABEL_UNSURE];
    __shared__ __attribute__((aligned(8))) uint8_t lab_t[128 * 24];   /* (row-major scans) [laser][firings of the tile + 8] */
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
            rec[e] = URF_FRONT128_RING_NONE;
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
        const bool on = ((bits >> e) & 1u) && (rec[e] & URF_FRONT128_RING_MASK) != URF_FRONT128_RING_NONE;
        const unsigned c = on ? (rec[e] & URF_FRONT128_RING_MASK) : 0u;
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
        const bool on = roi && (rec[e] & URF_FRONT128_RING_MASK) != URF_FRONT128_RING_NONE;
        const unsigned c = rec[e] & URF_FRONT128_RING_MASK;
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

#endif /* URF_FRONT128_FINISH_HPP */
