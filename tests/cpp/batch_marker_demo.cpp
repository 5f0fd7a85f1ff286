/* road_marker for a drive, three ways: urf::Detector message by message, urf::BatchDetector in batches of 2, and in batches of
 * 4 + the rest.  Each run's MarkerArrays are written in marker_demo's binary format; what that format does not carry
 * (frame_id, type, scale, orientation, position) is compared here, against Detector's, and a difference fails the run.
 * simple_poly_allow = -1: neither detector is given marker parameters (both must start from urf_default_marker_params).
 *   usage: batch_marker_demo simple_poly_allow poly_z_avg_allow out_detector.bin out_batch2.bin out_batch4.bin cloud.bin [cloud.bin ...]
 *   cloud.bin: u32 n, float x[n], y[n], z[n]
 *   out: per message { u32 published, u32 n_markers, n_markers x { i32 id, action, type; f32 rgba[4]; u32 n_points; f64 xyz[n_points][3] } } */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "detector.hpp"

static void dump(FILE* f, const urf::MarkerArray* ma)
{
    const uint32_t pub = ma ? 1u : 0u, nm = ma ? (uint32_t)ma->markers.size() : 0u;
    std::fwrite(&pub, 4, 1, f);
    std::fwrite(&nm, 4, 1, f);
    for (uint32_t m = 0; m < nm; m++) {
        const urf::Marker& mk = ma->markers[m];
        const int32_t ia[3] = { mk.id, mk.action, mk.type };
        const uint32_t np = (uint32_t)mk.points.size();
        std::fwrite(ia, 4, 3, f);
        std::fwrite(mk.color.data(), 4, 4, f);
        std::fwrite(&np, 4, 1, f);
        for (const auto& q : mk.points)
            std::fwrite(q.data(), 8, 3, f);
    }
}

static bool same_rest(const urf::MarkerArray* a, const urf::MarkerArray* b)
{
    if (!a || !b)
        return !a && !b;
    if (a->markers.size() != b->markers.size())
        return false;
    for (size_t m = 0; m < a->markers.size(); m++) {
        const urf::Marker &x = a->markers[m], &y = b->markers[m];
        if (x.frame_id != y.frame_id || x.type != y.type || x.scale != y.scale || x.orientation != y.orientation || x.position != y.position)
            return false;
    }
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 7)
        return 2;
    urf_marker_params mp;
    urf_default_marker_params(&mp);
    const bool set_mp = atoi(argv[1]) >= 0;
    mp.simple_poly_allow = atoi(argv[1]);
    mp.poly_z_avg_allow = atoi(argv[2]);
    const uint32_t n_max = 64 * 2048;
    const char* frame = "map_frame";
    std::vector<urf::PointCloud2> msgs;
    for (int k = 6; k < argc; k++) {
        FILE* fi = std::fopen(argv[k], "rb");
        uint32_t n = 0;
        if (!fi || std::fread(&n, 4, 1, fi) != 1 || n > n_max)
            return 3;
        std::vector<float> x(n), y(n), z(n);
        if (std::fread(x.data(), 4, n, fi) != n || std::fread(y.data(), 4, n, fi) != n || std::fread(z.data(), 4, n, fi) != n)
            return 3;
        std::fclose(fi);
        urf::PointCloud2 m;   /* x y z FLOAT32, 16-byte records */
        m.width = n;
        m.point_step = 16;
        m.row_step = 16 * n;
        const char* names[3] = { "x", "y", "z" };
        for (uint32_t a = 0; a < 3; a++) {
            urf::PointField fld;
            fld.name = names[a];
            fld.offset = 4 * a;
            fld.datatype = urf::PointField::FLOAT32;
            m.fields.push_back(fld);
        }
        m.data.resize((size_t)16 * n);
        for (uint32_t i = 0; i < n; i++) {
            const float rec[4] = { x[i], y[i], z[i], 0.f };
            std::memcpy(m.data.data() + (size_t)16 * i, rec, 16);
        }
        m.header.seq = (uint32_t)(k - 6);
        msgs.push_back(m);
    }
    try {
        std::vector<urf::MarkerArray> ref(msgs.size());
        std::vector<char> ref_pub(msgs.size(), 0);
        {
            urf::Detector det(0, n_max);
            urf_params p = det.params();
            p.min_X = p.min_Y = -200.f;
            p.max_X = p.max_Y = 200.f;
            det.setParams(p);
            det.enableRoadMarker(true, frame);
            if (set_mp)
                det.setMarkerParams(mp);
            FILE* f = std::fopen(argv[3], "wb");
            for (size_t i = 0; i < msgs.size(); i++) {
                det.filtered(msgs[i]);
                const urf::MarkerArray* ma = det.road_marker();
                dump(f, ma);
                ref_pub[i] = ma != nullptr;
                if (ma)
                    ref[i] = *ma;
            }
            std::fclose(f);
        }
        const size_t first[2] = { 2, 4 };
        for (int run = 0; run < 2; run++) {
            urf::BatchDetector det(0, n_max, 8);
            urf_params p = det.params();
            p.min_X = p.min_Y = -200.f;
            p.max_X = p.max_Y = 200.f;
            det.setParams(p);
            det.enableRoadMarker(true, frame);
            if (set_mp)
                det.setMarkerParams(mp);
            FILE* f = std::fopen(argv[4 + run], "wb");
            for (size_t s0 = 0; s0 < msgs.size();) {
                /* run 0: batches of 2; run 1: 4, then the rest */
                const size_t k = std::min(msgs.size() - s0, run == 0 ? first[0] : (s0 == 0 ? first[1] : msgs.size()));
                const std::vector<urf::PointCloud2> part(msgs.begin() + s0, msgs.begin() + s0 + k);
                det.filtered(part);
                for (size_t i = 0; i < k; i++) {
                    dump(f, det.road_marker(i));
                    if (!same_rest(det.road_marker(i), ref_pub[s0 + i] ? &ref[s0 + i] : nullptr)) {
                        std::fprintf(stderr, "message %zu: header / type / scale / pose differ from Detector's\n", s0 + i);
                        return 4;
                    }
                }
                s0 += k;
            }
            std::fclose(f);
        }
    } catch (const urf::Error& e) {
        std::fprintf(stderr, "urf error %d: %s\n", e.code, e.what());
        return 1;
    }
    return 0;
}
