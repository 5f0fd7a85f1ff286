/*
 * urf_k_front_sectors.hpp -- k_front_sectors: the sector half of k_split's stable multi-split for the tiles of a fused scan whose firings
 * span several star sectors (urf_set_front_multi_sector; k_front*_ms, urf_front.hpp).
 *
 * What k_front*_ms leaves per tile: the star records (sr, sz, sslot) of the tile's participants compacted in INPUT order from the tile's
 * base on, the 16-bit sector of each in the same place of front_skey, and the participants' count in tsoff[row][K].  What k_index, the
 * sort kernels, k_star_ties, the walks, k_front_finish, k_label_front and the read-outs expect: the records ordered by sector, input
 * order inside a sector, and tsoff[row][k] = first record of sector k in the tile, [K] = the count.  This kernel makes the one from the
 * other, in place.
 *
 * Grid (tiles, scans) x 256 threads.  Wave w owns the records [w * 512, w * 512 + 512) of the tile, 64 per step, eight steps.  A record's
 * rank inside its sector =
 *     records of that sector in earlier waves                (LDS matrix wcnt[wave][sector], scanned per sector)
 *   + ... in earlier steps of its own wave                   (running value of wcnt[wave][sector])
 *   + ... in lower lanes of its own step                     (match_any + popcount),
 * its place = records of smaller sectors (the scan across the sectors: tsoff) + rank.  Counts and prefixes only: no atomic decides an
 * order, and any keys in [0, K) are put in order, not only the few runs a sensor produces.  The workgroup holds the tile's records in
 * registers (eight per thread) across the barriers between the last load and the first store.  A tile whose records are in order already
 * -- every tile of a sweep without azimuth offsets -- gets its tsoff row and no store besides.
 *
 * A scan with front_ok[s] == 0 belongs to the general kernels (k_split has written its tsoff and records): the workgroup returns at once.
 * LDS: 4 x 1024 counts of 16 bits, 1024 + 8 words: 12.3 KB per workgroup.
 */
#ifndef URF_K_FRONT_SECTORS_HPP
#define URF_K_FRONT_SECTORS_HPP

#define URF_FSEC_THREADS 256u
#define URF_FSEC_WAVES (URF_FSEC_THREADS / 64u)
#define URF_FSEC_Q (URF_TILE / URF_FSEC_THREADS)   /* records per thread */
#define URF_FSEC_KEYS 1024u                        /* sectors the tables hold: URF_MAX_SECTORS and the total */
static_assert(URF_MAX_SECTORS + 1u <= URF_FSEC_KEYS && URF_FSEC_KEYS == 4u * URF_FSEC_THREADS, "four sectors per thread; [K] holds the total");

__global__ __launch_bounds__(URF_FSEC_THREADS) void k_front_sectors(urf_kargs a, urf_dev_params dp)
{
    __shared__ uint16_t wcnt[URF_FSEC_WAVES][URF_FSEC_KEYS];
    __shared__ unsigned soff[URF_FSEC_KEYS];
    __shared__ unsigned wsum[URF_FSEC_WAVES], moved;
    const unsigned s = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    if (a.front_ok[s] == 0u)
        return;   /* (uniform) the general kernels' scan */
    unsigned off, len;
    urf_scan_range(a, s, off, len);
    if (t * URF_TILE >= len)
        return;
    const unsigned K = (unsigned)dp.p.sectors;
    const size_t row = (size_t)s * a.tiles + t;
    uint16_t* const trow = a.tsoff + row * (K + 1);
    const unsigned n_raw = trow[K];   /* the tile's participants (k_front*_ms: tile_end) */
    const unsigned n = n_raw < URF_TILE ? n_raw : URF_TILE;
    const unsigned tb = urf_sbase(a, s) + t * URF_TILE;
    float* const g_sr = a.sr + tb;
    float* const g_sz = a.sz + tb;
    uint16_t* const g_ss = a.sslot + tb;
    const uint16_t* const g_sk = a.front_skey + tb;

    unsigned key[URF_FSEC_Q], ss[URF_FSEC_Q];
    float r[URF_FSEC_Q], z[URF_FSEC_Q];
#pragma unroll
    for (unsigned q = 0; q < URF_FSEC_Q; q++) {
        const unsigned i = wave * (URF_FSEC_Q * 64u) + q * 64u + lane, j = i < n ? i : 0u;
        const unsigned k = g_sk[j];
        key[q] = k < K ? k : K - 1u;   /* (the march writes sectors below K only: nothing indexes beyond the tables) */
        r[q] = g_sr[j];
        z[q] = g_sz[j];
        ss[q] = g_ss[j];
    }
    for (unsigned k = tid; k < URF_FSEC_WAVES * URF_FSEC_KEYS / 2u; k += URF_FSEC_THREADS)
        ((unsigned*)&wcnt[0][0])[k] = 0u;
    if (tid == 0)
        moved = 0u;
    __syncthreads();
    /* ranks inside the wave's own 512 records: the lanes of a step that share a sector read its running count (one address: a
     * broadcast), the first of them adds the group's size; a wave touches only its own row, in program order */
    uint16_t* const my = wcnt[wave];
    unsigned rank[URF_FSEC_Q];
#pragma unroll
    for (unsigned q = 0; q < URF_FSEC_Q; q++) {
        const bool on = wave * (URF_FSEC_Q * 64u) + q * 64u + lane < n;
        const unsigned long long m = urf_match_any_on(key[q], on, dp.sec_keybits);
        const unsigned old = my[on ? key[q] : 0u];
        if (on && urf_is_leader(m))
            my[key[q]] = (uint16_t)(old + (unsigned)__popcll(m));
        rank[q] = old + urf_popc_below(m);
    }
    __syncthreads();
    /* per sector the exclusive scan of its counts over the waves, then -- by the same thread -- the scan across the sectors: four
     * sectors per thread */
    unsigned v[4], sum = 0;
#pragma unroll
    for (unsigned e = 0; e < 4u; e++) {
        const unsigned k = tid * 4u + e;
        unsigned run = 0;
#pragma unroll
        for (unsigned w = 0; w < URF_FSEC_WAVES; w++) {
            const unsigned c = wcnt[w][k];
            wcnt[w][k] = (uint16_t)run;
            run += c;
        }
        v[e] = k < K ? run : 0u;
        sum += v[e];
    }
    const unsigned inc = urf_wave_scan_add(sum);
    if (lane == 63u)
        wsum[wave] = inc;
    __syncthreads();
    {
        unsigned run = inc - sum;
#pragma unroll
        for (unsigned w = 0; w < URF_FSEC_WAVES; w++)
            run += w < wave ? wsum[w] : 0u;
#pragma unroll
        for (unsigned e = 0; e < 4u; e++) {
            soff[tid * 4u + e] = run;   /* (the entries from K on: the total) */
            run += v[e];
        }
    }
    __syncthreads();
    /* the records' places; the tile's run table */
    unsigned pos[URF_FSEC_Q];
    bool any = false;
#pragma unroll
    for (unsigned q = 0; q < URF_FSEC_Q; q++) {
        const unsigned i = wave * (URF_FSEC_Q * 64u) + q * 64u + lane;
        pos[q] = soff[key[q]] + my[key[q]] + rank[q];
        any = any | (i < n && pos[q] != i);
    }
    if (any)
        moved = 1u;   /* (every writer writes the same value) */
    for (unsigned k = tid; k <= K; k += URF_FSEC_THREADS)
        trow[k] = (uint16_t)soff[k];
    __syncthreads();
    if (moved == 0u)
        return;   /* (uniform) the sectors of the tile do not fall: the records stay where they are */
#pragma unroll
    for (unsigned q = 0; q < URF_FSEC_Q; q++) {
        const unsigned i = wave * (URF_FSEC_Q * 64u) + q * 64u + lane;
        if (i < n && pos[q] < n) {   /* (a permutation of [0, n): the second test never fails) */
            g_sr[pos[q]] = r[q];
            g_sz[pos[q]] = z[q];
            g_ss[pos[q]] = (uint16_t)ss[q];
        }
    }
}

#endif /* URF_K_FRONT_SECTORS_HPP */
