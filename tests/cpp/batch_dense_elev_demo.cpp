/* urf::BatchDetector::setDenseElevations: dense messages WITHOUT a `ring` field (pcl::PointXYZI, what the reference subscribes to)
 * through BatchDetector::filtered three times -- as today (urf_classify_batch_pc2_ragged), with setDenseRealign + setDenseElevations
 * (urf_classify_batch_pc2_dense_elev: the ids derived from the points' elevation on the device), and with setDenseRealign alone --
 * must give the same four clouds, headers, summaries and road_marker arrays, byte for byte; denseAligned() == the message count with the
 * table, 0 without it.  Links the PRODUCT library only.  Built and run by tests/test_gpu_dense_elev.py.
 *   usage: batch_dense_elev_demo clouds.bin
 *   clouds.bin: u32 k, u32 lasers, u32 max_firings, float elev[lasers], then k times { u32 n, float x[n], y[n], z[n], intensity[n] }
 *   stdout: "elev messages <k> published <p> points <m> equal <e> aligned <a>", "plain messages <k> equal <e> aligned <a>",
 *           "cleared messages <k> equal <e> aligned <a>", "done" */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detector.hpp"

struct Cloud {
    std::vector<float> x, y, z, in;
};

static urf::PointField field(const char* name, uint32_t off, uint8_t type)
{
    urf::PointField f;
    f.name = name;
    f.offset = off;
    f.datatype = type;
    return f;
}

/* pcl::PointXYZI on the wire: x y z (pad) intensity (pad), 32 bytes */
static urf::PointCloud2 message(const Cloud& c, uint32_t seq)
{
    const uint32_t n = (uint32_t)c.x.size();
    urf::PointCloud2 m;
    m.header.seq = seq;
    m.header.stamp = 1000000ull * seq + 7;
    m.header.frame_id = "velodyne";
    m.width = n;
    m.is_dense = true;
    m.point_step = 32;
    const uint8_t F = urf::PointField::FLOAT32;
    m.fields = { field("x", 0, F), field("y", 4, F), field("z", 8, F), field("intensity", 16, F) };
    m.data.assign((size_t)n * 32, 0);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t* r = &m.data[(size_t)i * 32];
        std::memcpy(r + 0, &c.x[i], 4);
        std::memcpy(r + 4, &c.y[i], 4);
        std::memcpy(r + 8, &c.z[i], 4);
        std::memcpy(r + 16, &c.in[i], 4);
    }
    m.row_step = m.point_step * n;
    return m;
}

static bool same(const urf::PointCloud& a, const urf::PointCloud& b)
{
    return a.header.seq == b.header.seq && a.header.stamp == b.header.stamp && a.header.frame_id == b.header.frame_id &&
           a.points.size() == b.points.size() &&
           (a.points.empty() || std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(urf::PointXYZI)) == 0);
}

static bool same(const urf::MarkerArray* a, const urf::MarkerArray* b)
{
    if (!a || !b)
        return !a && !b;
    if (a->markers.size() != b->markers.size())
        return false;
    for (size_t m = 0; m < a->markers.size(); m++) {
        const urf::Marker &x = a->markers[m], &y = b->markers[m];
        if (x.frame_id != y.frame_id || x.type != y.type || x.action != y.action || x.id != y.id || x.scale != y.scale ||
            x.orientation != y.orientation || x.position != y.position || x.color != y.color || x.points != y.points)
            return false;
    }
    return true;
}

static size_t equal_messages(const urf::BatchDetector& a, const urf::BatchDetector& b, size_t k, size_t& points)
{
    size_t equal = 0;
    points = 0;
    for (size_t i = 0; i < k; i++) {
        bool eq = a.size() == k && b.size() == k && a.published(i) == b.published(i);
        eq = eq && same(a.road(i), b.road(i)) && same(a.curb(i), b.curb(i)) && same(a.roi(i), b.roi(i)) && same(a.road_probably(i), b.road_probably(i));
        eq = eq && std::memcmp(&a.info(i), &b.info(i), sizeof(urf_scan_info)) == 0 && same(a.road_marker(i), b.road_marker(i));
        equal += eq;
        points += b.roi(i).points.size() + b.road(i).points.size() + b.curb(i).points.size() + b.road_probably(i).points.size();
        if (!eq)
            std::printf("mismatch message %zu\n", i);
    }
    return equal;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi)
        return 3;
    uint32_t head[3] = { 0, 0, 0 };
    if (std::fread(head, 4, 3, fi) != 3)
        return 3;
    const uint32_t k = head[0], lasers = head[1], max_firings = head[2];
    if (lasers == 0 || lasers > 128)
        return 3;
    std::vector<float> elev(lasers);
    if (std::fread(elev.data(), 4, lasers, fi) != lasers)
        return 3;
    std::vector<Cloud> clouds(k);
    for (auto& c : clouds) {
        uint32_t n = 0;
        if (std::fread(&n, 4, 1, fi) != 1)
            return 3;
        for (auto* v : { &c.x, &c.y, &c.z, &c.in }) {
            v->resize(n);
            if (n && std::fread(v->data(), 4, n, fi) != n)
                return 3;
        }
    }
    std::fclose(fi);
    try {
        const uint32_t max_n = lasers * max_firings;
        urf::BatchDetector ragged(0, max_n, k), dense(0, max_n, k);
        urf_params p = ragged.params();
        p.min_X = p.min_Y = -200.f;
        p.max_X = p.max_Y = 200.f;
        p.channels = (int32_t)lasers;
        ragged.setParams(p);
        dense.setParams(p);
        ragged.enableRoadMarker(true, "map_frame");
        dense.enableRoadMarker(true, "map_frame");
        dense.setDenseRealign(max_firings);
        std::vector<urf::PointCloud2> msgs;
        for (uint32_t i = 0; i < k; i++)
            msgs.push_back(message(clouds[i], i));
        /* 0: realignment alone (as before this switch), 1: with the table, 2: the table cleared again */
        for (int round = 0; round < 3; round++) {
            if (round == 1)
                dense.setDenseElevations(elev);
            if (round == 2)
                dense.setDenseElevations({});
            const size_t published = ragged.filtered(msgs);
            const size_t published_d = dense.filtered(msgs);
            size_t points = 0;
            const size_t equal = published == published_d ? equal_messages(ragged, dense, k, points) : 0;
            if (round == 1)
                std::printf("elev messages %u published %zu points %zu equal %zu aligned %zu\n", k, published_d, points, equal, dense.denseAligned());
            else
                std::printf("%s messages %u equal %zu aligned %zu\n", round == 0 ? "plain" : "cleared", k, equal, dense.denseAligned());
        }
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("done\n");
    return 0;
}
