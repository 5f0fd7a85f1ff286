/* marker.cpp -- see marker.hpp. */
#include "marker.hpp"

#include <cstring>

namespace urf {

namespace {
float segmentDistance2(const std::array<float, 2>& p, const std::array<float, 2>& a, const std::array<float, 2>& b)
{
    const float vx = b[0] - a[0], vy = b[1] - a[1];
    const float wx = p[0] - a[0], wy = p[1] - a[1];
    const float c1 = wx * vx + wy * vy;
    if (c1 <= 0.0f)
        return wx * wx + wy * wy;
    const float c2 = vx * vx + vy * vy;
    if (c2 <= c1) {
        const float ux = p[0] - b[0], uy = p[1] - b[1];
        return ux * ux + uy * uy;
    }
    const float t = c1 / c2;
    const float qx = a[0] + t * vx, qy = a[1] + t * vy;
    const float dx = p[0] - qx, dy = p[1] - qy;
    return dx * dx + dy * dy;
}

void simplifySpan(const std::vector<std::array<float, 2>>& line, size_t a, size_t b, float tol2, std::vector<char>& keep)
{
    if (b < a + 2)
        return;
    float far2 = -1.0f;
    size_t arg = a;
    for (size_t i = a + 1; i < b; ++i) {
        const float d2 = segmentDistance2(line[i], line[a], line[b]);
        if (d2 > far2) {
            far2 = d2;
            arg = i;
        }
    }
    if (far2 > tol2) {
        keep[arg] = 1;
        simplifySpan(line, a, arg, tol2, keep);
        simplifySpan(line, arg, b, tol2, keep);
    }
}
}   // namespace

std::vector<std::array<float, 2>> simplifyLine(const std::vector<std::array<float, 2>>& line, float tolerance)
{
    if (line.size() < 3 || tolerance < 0.0f)
        return line;
    std::vector<char> keep(line.size(), 0);
    keep.front() = keep.back() = 1;
    simplifySpan(line, 0, line.size() - 1, tolerance * tolerance, keep);
    std::vector<std::array<float, 2>> out;
    for (size_t i = 0; i < line.size(); ++i)
        if (keep[i])
            out.push_back(line[i]);
    return out;
}

}   // namespace urf

/* C view of simplifyLine (include/urf.h): known-answer tests bind it without a C++ compiler */
extern "C" int urf_simplify_line(const float* xy, uint32_t n, float max_distance, uint8_t* keep)
{
    if ((!xy || !keep) && n)
        return URF_ERR_INVALID_ARG;
    std::vector<std::array<float, 2>> line(n);
    for (uint32_t i = 0; i < n; i++)
        line[i] = { xy[2 * i], xy[2 * i + 1] };
    const auto out = urf::simplifyLine(line, max_distance);
    size_t k = 0;   /* the result is a subsequence of the input: mark its members */
    for (uint32_t i = 0; i < n; i++) {
        keep[i] = k < out.size() && out[k] == line[i];
        k += keep[i];
    }
    return k == out.size() ? URF_OK : URF_ERR_INVALID_ARG;
}

namespace urf {

namespace {
/* lidar_segmentation.cpp:471-489 (and :508-526, :544-562): the strip whose points are the marker points a .. b (a joint
 * point belongs to both of its strips), optionally replaced by the simplified outline at the manual height */
void closeStrip(const float* pts, int a, int b, int id, bool red, const urf_marker_params& mp, urf_marker_strip* strips, uint32_t& ns,
                float* xyz, uint32_t& np)
{
    urf_marker_strip& m = strips[ns++];
    m.id = id;
    m.action = URF_MARKER_ADD;
    m.r = red ? 1.f : 0.f;
    m.g = red ? 0.f : 1.f;
    m.b = 0.f;
    m.a = 1.f;
    m.first_point = np;
    if (mp.simple_poly_allow) {
        std::vector<std::array<float, 2>> line;
        for (int i = a; i <= b; ++i)
            line.push_back({ { pts[4 * i], pts[4 * i + 1] } });
        for (const auto& q : simplifyLine(line, mp.poly_s_param)) {
            xyz[3 * np] = q[0];
            xyz[3 * np + 1] = q[1];
            xyz[3 * np + 2] = mp.poly_z_manual;
            ++np;
        }
    } else {
        for (int i = a; i <= b; ++i, ++np)
            std::memcpy(xyz + 3 * np, pts + 4 * i, 3 * sizeof(float));
    }
    m.n_points = np - m.first_point;
}
}   // namespace

/* lidar_segmentation.cpp:369-602 for one sweep; the one implementation behind urf_marker_strips and MarkerBuilder::build.
 * The reference appends point after point to the current strip and to its member linestring and closes both at a colour
 * change; as the last two points share their colour after the fix-ups, the last strip is always closed on the
 * i == cM - 1 path (:456-490) and the linestring is empty between sweeps.  So a strip is a range of
 * marker points: strip k runs from joint k to joint k + 1, where the joint of a colour change at i is i - 1 when the new
 * run is red and i when it is green (the joining segment is red, :495-577). */
int buildMarkerStrips(const float* pts, uint32_t k, const urf_marker_params& mp, int32_t* ghostcount, int32_t* published,
                      urf_marker_strip* strips, uint32_t* n_strips, float* xyz, uint32_t* n_points)
{
    *published = 0;
    *n_strips = *n_points = 0;
    if (k > URF_MARKER_MAX_POINTS)
        return URF_ERR_INVALID_ARG;
    const int cM = (int)k;
    for (int i = 0; i < cM; ++i)
        if (pts[4 * i + 3] != 0.0f && pts[4 * i + 3] != 1.0f)
            return URF_ERR_INVALID_ARG;
    if (cM <= 2)   /* :371 */
        return URF_OK;
    float red[URF_MARKER_MAX_POINTS];
    for (int i = 0; i < cM; ++i)
        red[i] = pts[4 * i + 3];
    /* :379-415: a point needs a neighbour of its own colour */
    if (red[0] == 0 && red[1] == 1) red[0] = 1;
    if (red[cM - 1] == 0 && red[cM - 2] == 1) red[cM - 1] = 1;
    if (red[0] == 1 && red[1] == 0) red[0] = 0;
    if (red[cM - 1] == 1 && red[cM - 2] == 0) red[cM - 1] = 0;
    for (int i = 2; i <= cM - 3; ++i)
        if (red[i] == 0 && red[i - 1] == 1 && red[i + 1] == 1) red[i] = 1;
    for (int i = 2; i <= cM - 3; ++i)
        if (red[i] == 1 && red[i - 1] == 0 && red[i + 1] == 0) red[i] = 0;

    float zavg = 0.0f;
    int stripId = 0, start = 0;
    uint32_t ns = 0, np = 0;
    for (int i = 0; i < cM; ++i) {   /* :430-579 */
        zavg *= (float)i;
        zavg = (float)((double)zavg + (double)pts[4 * i + 2]);
        zavg /= (float)(i + 1);
        if (i > 0 && red[i] != red[i - 1]) {
            const int joint = red[i] == 0 ? i : i - 1;   /* red -> green: the joining segment is still red (:495-529); green -> red (:534-577) */
            closeStrip(pts, start, joint, stripId++, red[i - 1] != 0, mp, strips, ns, xyz, np);
            start = joint;
        }
        if (i == cM - 1)   /* the last strip is only closed on this path (:456) */
            closeStrip(pts, start, i, stripId, red[i] != 0, mp, strips, ns, xyz, np);
    }
    if (mp.poly_z_avg_allow)   /* :580-589 */
        for (uint32_t q = 0; q < np; ++q)
            xyz[3 * q + 2] = zavg;
    int32_t ghost = *ghostcount < 0 ? 0 : (*ghostcount > URF_MARKER_MAX_STRIPS - 1 ? URF_MARKER_MAX_STRIPS - 1 : *ghostcount);
    for (int del = stripId; del < ghost; ++del) {   /* :591-598 obsolete markers of the previous sweep */
        strips[ns] = strips[ns - 1];
        strips[ns].id++;
        strips[ns].action = URF_MARKER_DELETE;
        strips[ns].first_point = np;
        strips[ns].n_points = 0;
        ++ns;
    }
    *ghostcount = stripId;
    *published = 1;
    *n_strips = ns;
    *n_points = np;
    return URF_OK;
}

}   // namespace urf

extern "C" int urf_marker_strips(const float* pts, uint32_t count, const urf_marker_params* mp, int32_t* ghostcount, int32_t* published,
                                 urf_marker_strip* strips, uint32_t* n_strips, float* xyz, uint32_t* n_points)
{
    if ((!pts && count) || !mp || mp->size != sizeof(urf_marker_params) || !ghostcount || !published || !strips || !n_strips || !xyz || !n_points)
        return URF_ERR_INVALID_ARG;
    return urf::buildMarkerStrips(pts, count, *mp, ghostcount, published, strips, n_strips, xyz, n_points);
}

namespace urf {

MarkerBuilder::MarkerBuilder() { urf_default_marker_params(&params_); }

bool MarkerBuilder::build(const float* pts, uint32_t k, MarkerArray& out)
{
    out.markers.clear();
    urf_marker_strip strips[URF_MARKER_MAX_STRIPS];   /* 12 KB of stack, no allocation */
    float xyz[3 * URF_MARKER_MAX_STRIP_POINTS];
    int32_t published = 0;
    uint32_t ns = 0, np = 0;
    if (buildMarkerStrips(pts, k, params_, &ghostcount_, &published, strips, &ns, xyz, &np) != URF_OK)
        throw Error(URF_ERR_INVALID_ARG, "MarkerBuilder::build: more than 361 marker points, or a colour that is neither 0 nor 1");
    if (!published)
        return false;
    toMarkerArray(strips, ns, xyz, fixed_frame_, out);
    return true;
}

void toMarkerArray(const urf_marker_strip* strips, uint32_t n_strips, const float* xyz, const std::string& fixed_frame, MarkerArray& out)
{
    out.markers.resize(n_strips);
    for (uint32_t m = 0; m < n_strips; ++m) {
        const urf_marker_strip& s = strips[m];
        Marker& mk = out.markers[m];
        mk = Marker();
        mk.frame_id = fixed_frame;
        mk.id = s.id;
        mk.action = s.action;
        mk.color = { { s.r, s.g, s.b, s.a } };
        mk.points.resize(s.n_points);
        for (uint32_t q = 0; q < s.n_points; ++q) {
            const float* p = xyz + 3 * (size_t)(s.first_point + q);
            mk.points[q] = { { (double)p[0], (double)p[1], (double)p[2] } };
        }
    }
}

}   // namespace urf
