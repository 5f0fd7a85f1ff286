/* urf::BatchDetector::setFrontAuto: a batch of a sensor model's sweeps through BatchDetector::filtered six times in front mode 2 with
 * setFrontAuto(true), and through a second detector with the switches the first one reports as applied set by hand.  The four clouds,
 * headers and summaries of every message must be the same, byte for byte, after every one of the six calls (labels are the same on the
 * fused and on the general kernels), and the first detector must have settled.  Links the PRODUCT library only.  Built and run by
 * tests/test_gpu_detector_front_auto.py.
 *   usage: detector_front_auto_demo clouds.bin
 *   clouds.bin: u32 k, u32 lasers, then k times { u32 n, float x[n], y[n], z[n] }
 *   stdout: "messages <k> calls 6 equal <e> phase <p> applied <hex> explained <n>"; exit status 0 iff e == 6 * k and p == URF_AUTO_SETTLED */
#include <cstdio>
#include <cstring>
#include <vector>

#include "detector.hpp"

struct Cloud {
    std::vector<float> x, y, z;
};

static urf::PointField field(const char* name, uint32_t off)
{
    urf::PointField f;
    f.name = name;
    f.offset = off;
    f.datatype = urf::PointField::FLOAT32;
    return f;
}

static urf::PointCloud2 message(const Cloud& c, uint32_t seq)
{
    const uint32_t n = (uint32_t)c.x.size();
    urf::PointCloud2 m;
    m.header.seq = seq;
    m.header.stamp = 1000000ull * seq + 7;
    m.header.frame_id = "lidar";
    m.width = n;
    m.is_dense = false;
    m.point_step = 16;
    m.fields = { field("x", 0), field("y", 4), field("z", 8), field("intensity", 12) };
    m.data.assign((size_t)n * 16, 0);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t* r = &m.data[(size_t)i * 16];
        const float in = (float)(i % 251);
        std::memcpy(r + 0, &c.x[i], 4);
        std::memcpy(r + 4, &c.y[i], 4);
        std::memcpy(r + 8, &c.z[i], 4);
        std::memcpy(r + 12, &in, 4);
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

/* what a call published, message by message */
struct Published {
    std::vector<urf::PointCloud> clouds;
    std::vector<urf_scan_info> infos;
};
static Published published_by(const urf::BatchDetector& d, size_t k)
{
    Published p;
    for (size_t i = 0; i < k; i++) {
        for (const urf::PointCloud* c : { &d.roi(i), &d.road(i), &d.curb(i), &d.road_probably(i) })
            p.clouds.push_back(*c);
        p.infos.push_back(d.info(i));
    }
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    uint32_t head[2] = { 0, 0 };
    if (!fi || std::fread(head, 4, 2, fi) != 2)
        return 3;
    const uint32_t k = head[0], lasers = head[1];
    std::vector<Cloud> clouds(k);
    uint32_t max_n = 0;
    for (auto& c : clouds) {
        uint32_t n = 0;
        if (std::fread(&n, 4, 1, fi) != 1)
            return 3;
        for (auto* v : { &c.x, &c.y, &c.z }) {
            v->resize(n);
            if (n && std::fread(v->data(), 4, n, fi) != n)
                return 3;
        }
        max_n = n > max_n ? n : max_n;
    }
    std::fclose(fi);
    const int CALLS = 6;
    try {
        std::vector<urf::PointCloud2> msgs;
        for (uint32_t i = 0; i < k; i++)
            msgs.push_back(message(clouds[i], i));
        urf::BatchDetector self(0, max_n, k), hand(0, max_n, k);
        urf_params p = self.params();
        p.min_X = p.min_Y = -200.f;
        p.max_X = p.max_Y = 200.f;
        p.channels = (int32_t)lasers;
        self.setParams(p);
        hand.setParams(p);
        self.setFrontMode(2);
        self.setFrontAuto(true);
        std::vector<Published> first;
        for (int call = 0; call < CALLS; call++) {
            self.filtered(msgs);
            first.push_back(published_by(self, k));
        }
        const urf_front_auto_info info = self.frontAuto();
        hand.setFrontLasers128((info.applied & URF_ADVICE_LASERS128) != 0);
        hand.setFrontLongSweeps((info.applied & URF_ADVICE_LONG_SWEEPS) != 0);
        hand.setFrontCurbPoints((info.applied & URF_ADVICE_CURB_POINTS) != 0);
        hand.setFrontMultiSector((info.applied & URF_ADVICE_MULTI_SECTOR) != 0);
        hand.setFrontMultiSectorCurbPoints((info.applied & URF_ADVICE_MULTI_SECTOR_CP) != 0);
        hand.setFrontMode((info.applied & URF_ADVICE_MODE_3) ? 3 : 2);
        size_t equal = 0;
        for (int call = 0; call < CALLS; call++) {
            hand.filtered(msgs);
            const Published b = published_by(hand, k);
            for (size_t i = 0; i < k; i++) {
                bool eq = std::memcmp(&first[call].infos[i], &b.infos[i], sizeof(urf_scan_info)) == 0;
                for (size_t c = 0; c < 4; c++)
                    eq = eq && same(first[call].clouds[i * 4 + c], b.clouds[i * 4 + c]);
                equal += eq;
                if (!eq)
                    std::printf("mismatch call %d message %zu\n", call, i);
            }
        }
        std::printf("messages %u calls %d equal %zu phase %u applied %#x explained %u\n", k, CALLS, equal, info.phase, info.applied, info.explained_calls);
        return equal == (size_t)CALLS * k && info.phase == URF_AUTO_SETTLED ? 0 : 1;
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
}
