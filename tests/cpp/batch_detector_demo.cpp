/* urf::BatchDetector against urf::Detector: a batch of wire messages of different lengths (one of them empty) through
 * BatchDetector::filtered, the same messages one by one through Detector::filtered, in both orders and three record
 * layouts; the four clouds of every message must be equal byte for byte, headers included.  Links the PRODUCT library only.
 * Built and run by tests/test_gpu_batch_clouds.py (and built without a GPU by tests/test_batch_clouds_cpu.py).
 *   usage: batch_detector_demo clouds.bin [default_roi]
 *   clouds.bin: u32 k, then k times { u32 n, float x[n], y[n], z[n], intensity[n] }
 *   stdout: one line per (layout, order): "layout <name> order <input|reference> messages <k> published <p> points <m> equal <e>"
 *           (e = messages whose four clouds and header equal Detector's), then "done" */
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

/* layout 0: pcl::PointXYZI (32 bytes: x y z w=1 intensity pad); 1: a permuted Ouster-like table (intensity z t x ring y, 32 bytes);
 * 2: 23-byte records without intensity (x at 3, y at 11, z at 17) */
static urf::PointCloud2 message(const Cloud& c, int layout, uint32_t seq)
{
    const uint32_t n = (uint32_t)c.x.size();
    urf::PointCloud2 m;
    m.header.seq = seq;
    m.header.stamp = 1000000ull * seq + 7;
    m.header.frame_id = "left_os1/os1_lidar";
    m.width = n;
    const uint8_t F = urf::PointField::FLOAT32;
    if (layout == 0) {
        m.point_step = 32;
        m.fields = { field("x", 0, F), field("y", 4, F), field("z", 8, F), field("intensity", 16, F) };
        m.data.resize((size_t)n * 32);
        for (uint32_t i = 0; i < n; i++) {
            const float rec[8] = { c.x[i], c.y[i], c.z[i], 1.0f, c.in[i], 0.f, 0.f, 0.f };
            std::memcpy(&m.data[(size_t)i * 32], rec, 32);
        }
    } else if (layout == 1) {
        m.point_step = 32;
        m.fields = { field("intensity", 0, F), field("z", 4, F), field("t", 8, urf::PointField::UINT32), field("x", 12, F),
                     field("ring", 16, urf::PointField::UINT16), field("y", 20, F) };
        m.data.resize((size_t)n * 32);
        for (uint32_t i = 0; i < n; i++) {
            float rec[8] = { c.in[i], c.z[i], 0.f, c.x[i], 0.f, c.y[i], 0.f, 0.f };
            const uint32_t t = 100u * i, ring = i % 64u;
            std::memcpy(&rec[2], &t, 4);
            std::memcpy(&rec[4], &ring, 4);
            std::memcpy(&m.data[(size_t)i * 32], rec, 32);
        }
    } else {
        m.point_step = 23;
        m.fields = { field("x", 3, F), field("y", 11, F), field("z", 17, F) };
        m.data.assign((size_t)n * 23, 0xa5);
        for (uint32_t i = 0; i < n; i++) {
            std::memcpy(&m.data[(size_t)i * 23 + 3], &c.x[i], 4);
            std::memcpy(&m.data[(size_t)i * 23 + 11], &c.y[i], 4);
            std::memcpy(&m.data[(size_t)i * 23 + 17], &c.z[i], 4);
        }
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

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi)
        return 3;
    uint32_t k = 0;
    if (std::fread(&k, 4, 1, fi) != 1)
        return 3;
    std::vector<Cloud> clouds(k);
    uint32_t max_n = 1;
    for (auto& c : clouds) {
        uint32_t n = 0;
        if (std::fread(&n, 4, 1, fi) != 1)
            return 3;
        for (auto* v : { &c.x, &c.y, &c.z, &c.in }) {
            v->resize(n);
            if (n && std::fread(v->data(), 4, n, fi) != n)
                return 3;
        }
        max_n = n > max_n ? n : max_n;
    }
    std::fclose(fi);
    try {
        urf::Detector det(0, max_n);
        urf::BatchDetector batch(0, max_n, k);
        urf_params p = det.params();
        if (!(argc > 2 && std::strcmp(argv[2], "default_roi") == 0)) {
            p.min_X = p.min_Y = -200.f;
            p.max_X = p.max_Y = 200.f;
        }
        det.setParams(p);
        batch.setParams(p);
        const char* names[3] = { "pointxyzi", "permuted", "step23" };
        for (int layout = 0; layout < 3; layout++) {
            std::vector<urf::PointCloud2> msgs;
            for (uint32_t i = 0; i < k; i++)
                msgs.push_back(message(clouds[i], layout, i));
            for (int ref = 0; ref < 2; ref++) {
                det.setReferenceOrder(ref != 0);
                batch.setReferenceOrder(ref != 0);
                const size_t published = batch.filtered(msgs);
                size_t equal = 0, points = 0;
                for (uint32_t i = 0; i < k; i++) {
                    const bool pub = det.filtered(msgs[i]);
                    bool eq = pub == batch.published(i) && batch.size() == k;
                    eq = eq && same(det.road(), batch.road(i)) && same(det.curb(), batch.curb(i)) && same(det.roi(), batch.roi(i)) &&
                         same(det.road_probably(), batch.road_probably(i));
                    eq = eq && det.info().status == batch.info(i).status && det.info().n_roi == batch.info(i).n_roi &&
                         det.info().n_road == batch.info(i).n_road && det.info().n_curb == batch.info(i).n_curb &&
                         det.info().n_ring10 == batch.info(i).n_ring10;
                    equal += eq;
                    points += batch.roi(i).points.size() + batch.road(i).points.size() + batch.curb(i).points.size() +
                              batch.road_probably(i).points.size();
                    if (!eq)
                        std::printf("mismatch layout %s order %d message %u\n", names[layout], ref, i);
                }
                std::printf("layout %s order %s messages %u published %zu points %zu equal %zu\n", names[layout],
                            ref ? "reference" : "input", k, published, points, equal);
            }
        }
        /* a batch whose messages do not share their layout is refused */
        {
            std::vector<urf::PointCloud2> mixed = { message(clouds[0], 0, 0), message(clouds[0], 2, 1) };
            try {
                batch.filtered(mixed);
                std::printf("mixed layouts accepted\n");
            } catch (const urf::Error& e) {
                std::printf("mixed layouts refused %d\n", e.code);
            }
        }
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
    std::printf("done\n");
    return 0;
}
