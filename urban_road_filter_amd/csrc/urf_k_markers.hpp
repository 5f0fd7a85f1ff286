/*
 * urf_k_markers.hpp -- road_marker: the line strips of a batch of sweeps, built on the device
 * (lidar_segmentation.cpp:369-602; host twin: buildMarkerStrips, marker.cpp; contract: urf_marker_strips_batch, include/urf.h).
 *
 * One wave per scan, the scan's at most 361 marker points in LDS.  The reference walks the points once and appends to the
 * strip at hand; here a strip is a RANGE of marker points -- strip k runs from joint k to joint k + 1, the joint of a colour
 * change at i being i - 1 when the new run is red and i when it is green (the joining segment is red, :495-577) -- so that
 * everything but two chains is a lane-parallel pass over the points:
 *   colours     the fix-ups (:381-415) make the ends copy their neighbours, then fill single green points between red ones,
 *               then single red points between green ones; each pass reads the previous pass's array (urf_mk_fixups says why
 *               that equals the reference's in-place loops)
 *   joints      prefix count of the colour changes: strip of every point, joint and colour of every strip
 *   keep flags  all points, or Douglas-Peucker per strip: spans on an explicit stack in LDS (at most 180 are ever open: they
 *               tile the strips' 360 segments and each holds two or more), the farthest point of a span by a wave-wide
 *               arg-max that reproduces the serial rule of marker.cpp (strict >, lowest index among equals, NaN never wins)
 *   zavg        the running mean of :436-438, a serial chain in the reference's own operation order (float *=, + through
 *               double, float /=), evaluated as such
 *   output      prefix count of the keep flags: point i of strip k lands at K(i) - 1 + k (k joints came before it, each
 *               written twice), a joint additionally in its other strip; one lane per marker record
 * The ghost chain: a scan needs the strip count of the nearest earlier scan that publishes.  It finds that scan from d_counts
 * alone (64 counts per step) and recomputes its colours; nobody waits for anybody.  Arithmetic: the library's flags
 * (-ffp-contract=off, IEEE division) hold here as everywhere; urf_mk_seg_dist2 is marker.cpp's segmentDistance2 operation
 * for operation.
 */
#ifndef URF_K_MARKERS_HPP
#define URF_K_MARKERS_HPP

#define URF_MK_PTS URF_MARKER_MAX_POINTS
#define URF_MK_STACK 192   /* >= 180 open spans (above) */

__device__ __forceinline__ float urf_mk_seg_dist2(float px, float py, float ax, float ay, float bx, float by)
{
    const float vx = bx - ax, vy = by - ay;
    const float wx = px - ax, wy = py - ay;
    const float c1 = wx * vx + wy * vy;
    if (c1 <= 0.0f)
        return wx * wx + wy * wy;
    const float c2 = vx * vx + vy * vy;
    if (c2 <= c1) {
        const float ux = px - bx, uy = py - by;
        return ux * ux + uy * uy;
    }
    const float t = c1 / c2;
    const float qx = ax + t * vx, qy = ay + t * vy;
    const float dx = px - qx, dy = py - qy;
    return dx * dx + dy * dy;
}

/* The colour fix-ups on c (n >= 3 colours, 0 green / 1 red), result in c; t is scratch of the same size.
 * Ends (:381-397): the four ordered statements only ever change c[0] and c[n - 1] and read c[1] and c[n - 2], which they
 * leave alone: whatever the values, the end takes its neighbour's colour.
 * 0 -> 1 pass (:399-406), in place in the reference, over i = 2 .. n - 3: c[i] = 1 if c[i] == 0 and both neighbours are 1.
 * The only updated value an iteration can see is c[i - 1]; that one was changed (0 -> 1) only if ITS right neighbour c[i] was 1,
 * and then iteration i changes nothing whichever value of c[i - 1] it reads.  So every iteration may read the array as it was
 * before the pass: a parallel pass from c to t.  The 1 -> 0 pass (:408-415) likewise, colours swapped, from t back to c. */
__device__ __forceinline__ void urf_mk_fixups(uint8_t* c, uint8_t* t, unsigned n, unsigned lane)
{
    if (lane == 0) {
        c[0] = c[1];
        c[n - 1] = c[n - 2];
    }
    urf_wave_lds_sync();
    for (unsigned i = lane; i < n; i += URF_WAVE) {
        uint8_t v = c[i];
        if (i >= 2 && i + 3 <= n && v == 0 && c[i - 1] == 1 && c[i + 1] == 1)
            v = 1;
        t[i] = v;
    }
    urf_wave_lds_sync();
    for (unsigned i = lane; i < n; i += URF_WAVE) {
        uint8_t v = t[i];
        if (i >= 2 && i + 3 <= n && v == 1 && t[i - 1] == 0 && t[i + 1] == 0)
            v = 0;
        c[i] = v;
    }
    urf_wave_lds_sync();
}

__device__ __forceinline__ unsigned urf_mk_count(const unsigned* d_counts, unsigned s)
{
    const unsigned n = d_counts[s];
    return n > URF_MK_PTS ? URF_MK_PTS : n;
}

__global__ __launch_bounds__(URF_WAVE) void k_marker_strips(const float* __restrict__ d_pts, const unsigned* __restrict__ d_counts, unsigned n_scans,
                                                            int sequence, urf_marker_params mp, const int* __restrict__ ghost_in,
                                                            int* __restrict__ ghost_out, urf_marker_strip* __restrict__ d_strips,
                                                            float* __restrict__ d_xyz, unsigned* __restrict__ d_n)
{
    __shared__ float px[URF_MK_PTS], py[URF_MK_PTS], pz[URF_MK_PTS];
    __shared__ uint8_t col[URF_MK_PTS + 3], tmp[URF_MK_PTS + 3], keep[URF_MK_PTS + 3];
    __shared__ uint16_t strip_of[URF_MK_PTS + 1];   /* colour changes at or before the point = its run's strip */
    __shared__ uint16_t kept[URF_MK_PTS + 1];       /* inclusive prefix count of keep */
    __shared__ uint16_t joint[URF_MARKER_MAX_STRIPS + 2];
    __shared__ uint8_t strip_red[URF_MARKER_MAX_STRIPS + 2];
    __shared__ uint16_t stack[2 * URF_MK_STACK];
    const unsigned s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_scans)
        return;
    const unsigned n = urf_mk_count(d_counts, s);
    const bool published = n > 2u;   /* :371 */
    const bool last = s + 1u == n_scans;
    if (!published && lane == 0) {
        d_n[3 * s] = 0u;
        d_n[3 * s + 1] = 0u;
        d_n[3 * s + 2] = 0u;
    }
    const bool chain = sequence != 0;
    if (!published && !(chain && last && ghost_out))
        return;

    /* ---- the ghost count this scan starts from: the strip count of the nearest earlier scan that publishes ---- */
    int ghost = 0, ghost_raw = 0;   /* ghost_raw: what an unpublished last scan hands on -- the incoming word as it came, as the host entry leaves it */
    if (chain) {
        int prev = -1;
        for (int base = (int)s - 1; base >= 0 && prev < 0; base -= URF_WAVE) {
            const int q = base - (int)lane;
            const unsigned long long m = __ballot(q >= 0 && d_counts[q] > 2u);
            if (m)
                prev = base - (__ffsll((long long)m) - 1);
        }
        if (prev < 0) {
            ghost = ghost_raw = ghost_in ? *ghost_in : 0;
            ghost = ghost < 0 ? 0 : (ghost > URF_MARKER_MAX_STRIPS - 1 ? URF_MARKER_MAX_STRIPS - 1 : ghost);
        } else {
            const unsigned np = urf_mk_count(d_counts, (unsigned)prev);
            const float* src = d_pts + (size_t)prev * URF_MK_PTS * 4;
            for (unsigned i = lane; i < np; i += URF_WAVE)
                col[i] = src[4 * i + 3] != 0.0f;
            urf_wave_lds_sync();
            urf_mk_fixups(col, tmp, np, lane);
            for (unsigned base = 0; base < np; base += URF_WAVE) {
                const unsigned i = base + lane;
                ghost += __popcll(__ballot(i >= 1 && i < np && col[i] != col[i - 1]));
            }
            ghost_raw = ghost;
            urf_wave_lds_sync();   /* col is loaded again below */
        }
    }
    if (!published) {   /* the last scan of a sequence: the count passes through it */
        if (lane == 0)
            *ghost_out = ghost_raw;
        return;
    }

    /* ---- this scan's points and colours ---- */
    const float* src = d_pts + (size_t)s * URF_MK_PTS * 4;
    for (unsigned i = lane; i < n; i += URF_WAVE) {
        px[i] = src[4 * i];
        py[i] = src[4 * i + 1];
        pz[i] = src[4 * i + 2];
        col[i] = src[4 * i + 3] != 0.0f;
    }
    urf_wave_lds_sync();
    urf_mk_fixups(col, tmp, n, lane);

    /* ---- joints ---- */
    unsigned n_changes = 0;
    for (unsigned base = 0; base < n; base += URF_WAVE) {
        const unsigned i = base + lane;
        const bool ch = i >= 1 && i < n && col[i] != col[i - 1];
        const unsigned k = n_changes + urf_wave_scan_add(ch ? 1u : 0u);
        if (i < n)
            strip_of[i] = (uint16_t)k;
        if (ch && k <= URF_MARKER_MAX_STRIPS - 1) {   /* (always: runs hold two points or more) */
            joint[k] = (uint16_t)(col[i] ? i - 1 : i);
            strip_red[k] = col[i];
        }
        n_changes += __popcll(__ballot(ch));
    }
    n_changes = n_changes > URF_MARKER_MAX_STRIPS - 1 ? URF_MARKER_MAX_STRIPS - 1 : n_changes;
    if (lane == 0) {
        joint[0] = 0;
        strip_red[0] = col[0];
        joint[n_changes + 1] = (uint16_t)(n - 1);
    }
    const bool simplify = mp.simple_poly_allow != 0;
    const bool keep_all = !simplify || mp.poly_s_param < 0.0f;   /* simplifyLine: a negative tolerance returns the line */
    for (unsigned i = lane; i < n; i += URF_WAVE)
        keep[i] = keep_all ? 1 : 0;
    urf_wave_lds_sync();

    /* ---- Douglas-Peucker per strip (marker.cpp simplifySpan) ---- */
    if (!keep_all) {
        for (unsigned k = lane; k <= n_changes + 1; k += URF_WAVE)
            keep[joint[k]] = 1;
        const float tol2 = mp.poly_s_param * mp.poly_s_param;
        for (unsigned k = 0; k <= n_changes; ++k) {
            unsigned top = 0;
            if (joint[k + 1] >= joint[k] + 2u) {
                if (lane == 0) {
                    stack[0] = joint[k];
                    stack[1] = joint[k + 1];
                }
                top = 1;
            }
            urf_wave_lds_sync();
            while (top > 0) {
                --top;
                const unsigned a = stack[2 * top], b = stack[2 * top + 1];
                urf_wave_lds_sync();   /* read before lane 0 pushes over it */
                const float ax = px[a], ay = py[a], bx = px[b], by = py[b];
                float far2 = -1.0f;
                unsigned arg = a;
                for (unsigned i = a + 1 + lane; i < b; i += URF_WAVE) {
                    const float d2 = urf_mk_seg_dist2(px[i], py[i], ax, ay, bx, by);
                    if (d2 > far2) {
                        far2 = d2;
                        arg = i;
                    }
                }
                /* a distance is a sum of squares: +0 .. +inf (NaN never got here), ordered like its bit pattern; 0 = no candidate */
                const unsigned code = far2 < 0.0f ? 0u : (urf_fbits(far2) & 0x7fffffffu) + 1u;
                const unsigned best = urf_wave_max(code);
                const unsigned at = urf_wave_min(code == best ? arg : 0xffffffffu);   /* lowest index among equal distances */
                if (best != 0u && __uint_as_float(best - 1u) > tol2) {
                    if (lane == 0) {
                        keep[at] = 1;
                        unsigned t = top;
                        if (at >= a + 2u && t < URF_MK_STACK) {
                            stack[2 * t] = (uint16_t)a;
                            stack[2 * t + 1] = (uint16_t)at;
                            ++t;
                        }
                        if (b >= at + 2u && t < URF_MK_STACK) {
                            stack[2 * t] = (uint16_t)at;
                            stack[2 * t + 1] = (uint16_t)b;
                        }
                    }
                    top += (at >= a + 2u && top < URF_MK_STACK) ? 1u : 0u;
                    top += (b >= at + 2u && top < URF_MK_STACK) ? 1u : 0u;
                }
                urf_wave_lds_sync();
            }
        }
    }

    /* ---- zavg (:436-438): the reference's chain, in its order; every lane runs it on the same values ---- */
    float zavg = 0.0f;
    if (mp.poly_z_avg_allow) {
        for (unsigned i = 0; i < n; ++i) {
            zavg *= (float)i;
            zavg = (float)((double)zavg + (double)pz[i]);
            zavg /= (float)(i + 1u);
        }
    }

    /* ---- positions and output ---- */
    unsigned n_kept = 0;
    for (unsigned base = 0; base < n; base += URF_WAVE) {
        const unsigned i = base + lane;
        const bool kp = i < n && keep[i] != 0;
        const unsigned k = n_kept + urf_wave_scan_add(kp ? 1u : 0u);
        if (i < n)
            kept[i] = (uint16_t)k;
        n_kept += __popcll(__ballot(kp));
    }
    urf_wave_lds_sync();
    const unsigned n_points = n_kept + n_changes;   /* every joint once more */
    float* xyz = d_xyz + (size_t)s * 3 * URF_MARKER_MAX_STRIP_POINTS;
    for (unsigned i = lane; i < n; i += URF_WAVE) {
        if (!keep[i])
            continue;
        const float z = mp.poly_z_avg_allow ? zavg : (simplify ? mp.poly_z_manual : pz[i]);
        const unsigned pos = (unsigned)kept[i] - 1u + strip_of[i];
        /* a green point next to a red run is a joint: also the last point of the red strip before it / the first of the one behind */
        const bool after_red = i >= 1 && col[i] == 0 && col[i - 1] == 1;
        const bool before_red = i + 1 < n && col[i] == 0 && col[i + 1] == 1;
        const unsigned lo = after_red ? pos - 1u : pos, hi = before_red ? pos + 1u : pos;
        for (unsigned q = lo; q <= hi && q < URF_MARKER_MAX_STRIP_POINTS; ++q) {
            xyz[3 * q] = px[i];
            xyz[3 * q + 1] = py[i];
            xyz[3 * q + 2] = z;
        }
    }
    urf_marker_strip* out = d_strips + (size_t)s * URF_MARKER_MAX_STRIPS;
    for (unsigned k = lane; k <= n_changes; k += URF_WAVE) {
        const unsigned a = joint[k], b = joint[k + 1];
        urf_marker_strip m;
        m.id = (int)k;
        m.action = URF_MARKER_ADD;
        m.r = strip_red[k] ? 1.0f : 0.0f;
        m.g = strip_red[k] ? 0.0f : 1.0f;
        m.b = 0.0f;
        m.a = 1.0f;
        m.first_point = (unsigned)kept[a] - 1u + k;
        m.n_points = (unsigned)kept[b] - (unsigned)kept[a] + 1u;
        out[k] = m;
    }
    /* :591-598: the previous sweep's strips n_changes + 1 .. ghost are gone (ghost <= URF_MARKER_MAX_STRIPS - 1: the records fit) */
    for (unsigned d = n_changes + lane; (int)d < ghost; d += URF_WAVE) {
        urf_marker_strip m;
        m.id = (int)d + 1;
        m.action = URF_MARKER_DELETE;
        m.r = strip_red[n_changes] ? 1.0f : 0.0f;
        m.g = strip_red[n_changes] ? 0.0f : 1.0f;
        m.b = 0.0f;
        m.a = 1.0f;
        m.first_point = n_points;
        m.n_points = 0u;
        out[d + 1] = m;
    }
    if (lane == 0) {
        d_n[3 * s] = 1u;
        d_n[3 * s + 1] = n_changes + 1u + ((int)n_changes < ghost ? (unsigned)ghost - n_changes : 0u);
        d_n[3 * s + 2] = n_points;
        if (chain && last && ghost_out)
            *ghost_out = (int)n_changes;
    }
}

#endif /* URF_K_MARKERS_HPP */
