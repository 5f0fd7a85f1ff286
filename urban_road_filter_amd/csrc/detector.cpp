/* detector.cpp -- see detector.hpp.  Host code; all classification happens behind the C ABI. */
#include "detector.hpp"

#include <hip/hip_runtime_api.h>

#include <cstring>

namespace urf {

Detector::Detector(int device, uint32_t max_points) : max_points_(max_points)
{
    /* four scratch rows: the slots of the asynchronous path get a row and a stream each */
    const int rc = urf_create(&ctx_, device, max_points, URF_MAX_IN_FLIGHT);
    if (rc != URF_OK)
        throw Error(rc, std::string("urf_create: ") + urf_strerror(rc));
}

Detector::~Detector()
{
    if (ctx_)
        urf_destroy(ctx_);
}

void Detector::check(int rc, const char* what) const
{
    if (rc < 0)
        throw Error(rc, std::string(what) + ": " + urf_strerror(rc) + " " + urf_last_error(ctx_));
}

void Detector::applySweepOutputs(bool sweep, bool marker, bool order)
{
    const uint32_t bits = sweep ? (marker ? URF_SWEEP_OUT_MARKER_POINTS : 0u) | (order ? URF_SWEEP_OUT_ORDER : 0u) : 0u;
    if (bits == sweep_bits_)
        return;   /* (a detector that never turns the switch on never calls the entry point) */
    check(urf_set_sweep_outputs(ctx_, bits), "urf_set_sweep_outputs");
    sweep_bits_ = bits;
}

void Detector::setSweepResultsDirect(bool on) { check(urf_set_sweep_results_direct(ctx_, on ? 1 : 0), "urf_set_sweep_results_direct"); }

void Detector::setSweepQuantum(uint32_t points) { check(urf_set_sweep_quantum(ctx_, points), "urf_set_sweep_quantum"); }

void Detector::setParams(const urf_params& p) { check(urf_set_params(ctx_, &p), "urf_set_params"); }

urf_params Detector::params() const
{
    urf_params p;
    check(urf_get_params(ctx_, &p), "urf_get_params");
    return p;
}

namespace {

/* point i of the message as a pcl::PointXYZI */
struct RecordsXYZI {   /* the message IS an array of pcl::PointXYZI (32 bytes, x y z at 0 / 4 / 8, intensity at 16) */
    const uint8_t* data;
    inline void get(uint32_t i, PointXYZI& out) const { std::memcpy(&out, data + (size_t)i * sizeof(PointXYZI), sizeof(PointXYZI)); }
};
struct RecordsAny {    /* any point_step and field offsets; intensity optional */
    const uint8_t* data;
    uint32_t step, ox, oy, oz;
    int64_t oi;
    inline void get(uint32_t i, PointXYZI& out) const
    {
        const uint8_t* p = data + (size_t)i * step;
        PointXYZI q;   /* pcl::PointXYZI's defaults for what the message does not carry */
        std::memcpy(&q.x, p + ox, 4);
        std::memcpy(&q.y, p + oy, 4);
        std::memcpy(&q.z, p + oz, 4);
        if (oi >= 0)
            std::memcpy(&q.intensity, p + oi, 4);
        out = q;
    }
};
struct RecordsXYZ_I {   /* x y z side by side and intensity right behind them (the layout of the Velodyne / Ouster drivers' messages) */
    const uint8_t* data;
    uint32_t step, ox;
    inline void get(uint32_t i, PointXYZI& out) const
    {
        const uint8_t* p = data + (size_t)i * step + ox;
        PointXYZI q;
        float v[4];
        std::memcpy(v, p, 16);
        q.x = v[0];
        q.y = v[1];
        q.z = v[2];
        q.intensity = v[3];
        out = q;
    }
};

/* lidar_segmentation.cpp:354-367, 605-608, 620: the four clouds from the label bytes, input order.  The clouds have
 * their final sizes already (the sweep's summary holds the four counts), so every point is ONE indexed store -- no
 * push_back, no capacity check; eight labels at a time: a region of interest that drops whole azimuth ranges leaves long
 * runs of zero bytes.  Returns false if the labels do not add up to the counts (cannot happen). */
template <class REC>
bool materialise(const REC& rec, const uint8_t* lab, uint32_t n, bool all_roi, bool lists, std::vector<PointXYZI>& roi,
                 std::vector<PointXYZI>& road, std::vector<PointXYZI>& curb, std::vector<PointXYZI>& probably)
{
    PointXYZI* const o_roi = roi.data();
    PointXYZI* const o_road = road.data();
    PointXYZI* const o_curb = curb.data();
    PointXYZI* const o_prob = probably.data();
    size_t k_roi = all_roi ? roi.size() : 0, k_road = 0, k_curb = 0, k_prob = 0;
    const size_t c_roi = roi.size(), c_road = lists ? road.size() : 0, c_curb = lists ? curb.size() : 0, c_prob = lists ? probably.size() : 0;
    bool ok = true;
    PointXYZI q;
    auto one = [&](uint32_t i, uint8_t l) {
        if (!(l & URF_FLAG_ROI))
            return;
        const bool need = !all_roi || (lists && (l & (URF_LABEL_MASK | URF_FLAG_RING10)));
        if (!need)
            return;
        rec.get(i, q);
        if (!all_roi) {
            if (k_roi < c_roi)
                o_roi[k_roi] = q;
            k_roi++;
        }
        if (lists) {
            if ((l & URF_LABEL_MASK) == URF_LABEL_ROAD) {
                if (k_road < c_road)
                    o_road[k_road] = q;
                k_road++;
            } else if ((l & URF_LABEL_MASK) == URF_LABEL_CURB) {
                if (k_curb < c_curb)
                    o_curb[k_curb] = q;
                k_curb++;
            }
            if (l & URF_FLAG_RING10) {
                if (k_prob < c_prob)
                    o_prob[k_prob] = q;
                k_prob++;
            }
        }
    };
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        std::memcpy(&w, lab + i, 8);
        if (w == 0)
            continue;
        for (uint32_t k = 0; k < 8; k++)
            one(i + k, (uint8_t)(w >> (8 * k)));
    }
    for (; i < n; i++)
        one(i, lab[i]);
    ok = k_roi == c_roi && (!lists || (k_road == c_road && k_curb == c_curb && k_prob == c_prob));
    return ok;
}

}   // namespace

void Detector::split(const Pending& m)
{
    road_.header = curb_.header = roi_.header = road_probably_.header = m.header;   /* lidar_segmentation.cpp:612-615 */
    marker_published_ = false;
    if (info_.status != URF_OK) {
        road_.points.clear();
        curb_.points.clear();
        roi_.points.clear();
        road_probably_.points.clear();
        return;
    }
    /* the clouds at their final sizes (a vector that shrinks or stays keeps its storage and initialises nothing: in a stream of
     * sweeps only growth beyond the largest sweep so far costs anything) */
    const bool lists = !reference_order_;   /* in the reference's order they come from the index lists below */
    roi_.points.resize(info_.n_roi);
    road_.points.resize(info_.n_road);
    curb_.points.resize(info_.n_curb);
    road_probably_.points.resize(info_.n_ring10);
    const uint32_t n = m.n;
    const bool xyzi = m.step == sizeof(PointXYZI) && m.ox == 0 && m.oy == 4 && m.oz == 8 && m.oi == 16;
    /* every point inside the region of interest and the message already an array of pcl::PointXYZI: "roi" is the message */
    const bool all_roi = xyzi && info_.n_roi == n && ((uintptr_t)m.data % alignof(PointXYZI)) == 0;
    if (all_roi)
        std::memcpy((void*)roi_.points.data(), m.data, (size_t)n * sizeof(PointXYZI));
    const bool xyz_i = !xyzi && m.oy == m.ox + 4 && m.oz == m.ox + 8 && m.oi == (int64_t)m.ox + 12 && (uint64_t)m.ox + 16 <= m.step;
    bool ok = true;
    if (all_roi && !lists)
        ;   /* nothing left for the label scan */
    else if (xyzi)
        ok = materialise(RecordsXYZI{ m.data }, labels_, n, all_roi, lists, roi_.points, road_.points, curb_.points, road_probably_.points);
    else if (xyz_i)
        ok = materialise(RecordsXYZ_I{ m.data, m.step, m.ox }, labels_, n, false, lists, roi_.points, road_.points, curb_.points,
                         road_probably_.points);
    else
        ok = materialise(RecordsAny{ m.data, m.step, m.ox, m.oy, m.oz, m.oi }, labels_, n, false, lists, roi_.points, road_.points, curb_.points,
                         road_probably_.points);
    if (!ok)
        throw Error(URF_ERR_HIP, "label bytes and summary counters disagree");
    if (marker_on_ && sweep_outputs_) {   /* the sweep brought them along (urf_set_sweep_outputs): the slot's pinned result buffer */
        const float* mp = nullptr;
        uint32_t k = 0;
        check(urf_result_marker_points(ctx_, m.ticket, &mp, &k), "urf_result_marker_points");
        marker_published_ = marker_.build(mp, k, markers_);
    } else if (marker_on_) {
        float mp[361 * 4];
        uint32_t k = 0;
        check(urf_marker_points(ctx_, 0, mp, &k), "urf_marker_points");
        marker_published_ = marker_.build(mp, k, markers_);
    }
    if (reference_order_) {
        const uint32_t *ro = nullptr, *co = nullptr, *po = nullptr;
        uint32_t cnt[3] = { 0, 0, 0 };
        if (sweep_outputs_) {
            check(urf_result_ordered_indices(ctx_, m.ticket, &ro, &co, &po, cnt), "urf_result_ordered_indices");
        } else {
            if (ord_.size() < 3 * (size_t)max_points_)
                ord_.resize(3 * (size_t)max_points_);   /* once */
            uint32_t* const wr = ord_.data();
            check(urf_ordered_indices(ctx_, 0, wr, wr + max_points_, wr + 2 * (size_t)max_points_, cnt), "urf_ordered_indices");
            ro = wr;
            co = wr + max_points_;
            po = wr + 2 * (size_t)max_points_;
        }
        const RecordsAny rec{ m.data, m.step, m.ox, m.oy, m.oz, m.oi };
        const RecordsXYZI recx{ m.data };
        PointXYZI q;
        auto fill = [&](std::vector<PointXYZI>& out, const uint32_t* idx, uint32_t c) {
            out.resize(c);   /* (= the summary's count) */
            PointXYZI* const o = out.data();
            for (uint32_t i = 0; i < c; i++) {
                if (xyzi)
                    recx.get(idx[i], q);
                else
                    rec.get(idx[i], q);
                o[i] = q;
            }
        };
        fill(road_.points, ro, cnt[0]);
        fill(curb_.points, co, cnt[1]);
        fill(road_probably_.points, po, cnt[2]);
    }
}

uint32_t Detector::submit(const uint8_t* data, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                          uint32_t off_z, const Header& header, int64_t off_intensity)
{
    if (off_intensity >= 0 && (uint64_t)off_intensity + 4 > point_step)
        throw Error(URF_ERR_INVALID_ARG, "intensity field outside the record");
    uint32_t t = 0;
    check(urf_classify_pc2_async(ctx_, data, n_points, point_step, off_x, off_y, off_z, &t), "urf_classify_pc2_async");
    Pending& m = pending_[t % URF_MAX_IN_FLIGHT];
    m.data = data;
    m.n = n_points;
    m.step = point_step;
    m.ox = off_x;
    m.oy = off_y;
    m.oz = off_z;
    m.oi = off_intensity;
    m.header = header;
    m.ticket = t;
    m.used = true;
    return t;
}

uint32_t Detector::submit(const PointCloud& cloud)
{
    return submit((const uint8_t*)cloud.points.data(), (uint32_t)cloud.points.size(), (uint32_t)sizeof(PointXYZI), 0, 4, 8,
                  cloud.header, 16);
}

bool Detector::collect(uint32_t ticket)
{
    Pending& m = pending_[ticket % URF_MAX_IN_FLIGHT];
    if (!m.used || m.ticket != ticket)
        throw Error(URF_ERR_INVALID_ARG, "collect: no such ticket in flight");
    m.used = false;
    check(urf_classify_pc2_wait(ctx_, ticket, nullptr, &info_), "urf_classify_pc2_wait");
    check(urf_result_labels(ctx_, ticket, &labels_), "urf_result_labels");   /* read in place: the slot's pinned result buffer */
    n_labels_ = m.n;
    split(m);
    return info_.status == URF_OK;
}

bool Detector::filtered(const PointCloud& cloud)
{
    if (cloud.points.empty()) {   /* (the C ABI refuses an empty message; the reference returns without publishing) */
        Pending m;
        m.header = cloud.header;
        info_ = urf_scan_info{};
        info_.status = URF_TOO_FEW_POINTS;
        labels_ = nullptr;
        n_labels_ = 0;
        split(m);
        return false;
    }
    return collect(submit(cloud));
}

bool Detector::filtered(const uint8_t* data, uint32_t n_points, uint32_t point_step,
                        uint32_t off_x, uint32_t off_y, uint32_t off_z, const Header& header, int64_t off_intensity)
{
    if (n_points == 0) {
        Pending m;
        m.header = header;
        info_ = urf_scan_info{};
        info_.status = URF_TOO_FEW_POINTS;
        labels_ = nullptr;
        n_labels_ = 0;
        split(m);
        return false;
    }
    return collect(submit(data, n_points, point_step, off_x, off_y, off_z, header, off_intensity));
}

/* pcl::fromROSMsg for pcl::PointXYZI: the fields x, y, z and intensity by name (FLOAT32), everything else ignored */
void Detector::resolve(const PointCloud2& msg, uint32_t off[3], int64_t& off_intensity, uint64_t& n)
{
    if (msg.is_bigendian)
        throw Error(URF_ERR_INVALID_ARG, "big-endian PointCloud2 is not supported");
    bool have[3] = { false, false, false };
    off_intensity = -1;
    for (const PointField& f : msg.fields) {
        for (int k = 0; k < 3; k++)
            if (f.name == (k == 0 ? "x" : k == 1 ? "y" : "z")) {
                if (f.datatype != PointField::FLOAT32)
                    throw Error(URF_ERR_INVALID_ARG, "field " + f.name + " is not FLOAT32");
                off[k] = f.offset;
                have[k] = true;
            }
        if (f.name == "intensity" && f.datatype == PointField::FLOAT32)   /* (another type: left at its default, as PCL does with a mismatching field) */
            off_intensity = (int64_t)f.offset;
    }
    if (!have[0] || !have[1] || !have[2])
        throw Error(URF_ERR_INVALID_ARG, "PointCloud2 without x/y/z fields");
    n = (uint64_t)msg.width * msg.height;
    if (msg.point_step < 4 || n * msg.point_step > msg.data.size() || n > 0xffffffffull)
        throw Error(URF_ERR_INVALID_ARG, "PointCloud2 data shorter than width*height*point_step");
}

uint32_t Detector::submit(const PointCloud2& msg)
{
    uint32_t off[3] = { 0, 0, 0 };
    int64_t oi = -1;
    uint64_t n = 0;
    resolve(msg, off, oi, n);
    return submit(msg.data.data(), (uint32_t)n, msg.point_step, off[0], off[1], off[2], msg.header, oi);
}

bool Detector::filtered(const PointCloud2& msg)
{
    uint32_t off[3] = { 0, 0, 0 };
    int64_t oi = -1;
    uint64_t n = 0;
    resolve(msg, off, oi, n);
    return filtered(msg.data.data(), (uint32_t)n, msg.point_step, off[0], off[1], off[2], msg.header, oi);
}

/* ---- BatchDetector ------------------------------------------------------------------------------------- */
BatchDetector::BatchDetector(int device, uint32_t max_points, uint32_t max_batch) : max_points_(max_points), max_batch_(max_batch), device_(device)
{
    urf_default_marker_params(&marker_params_);
    int rc = urf_create(&ctx_, device, max_points, max_batch);
    if (rc != URF_OK)
        throw Error(rc, std::string("urf_create: ") + urf_strerror(rc));
    hipStream_t st = nullptr;   /* the uploads, the library's kernels and the read-backs in one stream order */
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        urf_destroy(ctx_);
        ctx_ = nullptr;
        throw Error(URF_ERR_HIP, "BatchDetector: hipStreamCreate failed");
    }
    stream_ = st;
    rc = urf_set_stream(ctx_, st);
    if (rc != URF_OK) {
        urf_destroy(ctx_);
        ctx_ = nullptr;
        (void)hipStreamDestroy(st);
        throw Error(rc, std::string("urf_set_stream: ") + urf_strerror(rc));
    }
}

BatchDetector::~BatchDetector()
{
    if (ctx_)
        urf_destroy(ctx_);
    for (void* p : { d_data_, d_records_, d_small_, d_ghost_, d_marker_ })
        if (p)
            (void)hipFree(p);
    if (stream_)
        (void)hipStreamDestroy((hipStream_t)stream_);
}

void BatchDetector::check(int rc, const char* what) const
{
    if (rc < 0)
        throw Error(rc, std::string(what) + ": " + urf_strerror(rc) + " " + urf_last_error(ctx_));
}

void BatchDetector::setParams(const urf_params& p) { check(urf_set_params(ctx_, &p), "urf_set_params"); }

urf_params BatchDetector::params() const
{
    urf_params p;
    check(urf_get_params(ctx_, &p), "urf_get_params");
    return p;
}

void BatchDetector::enableRoadMarker(bool on, const std::string& fixed_frame)
{
    fixed_frame_ = fixed_frame;
    if (on && !d_ghost_ && (hipSetDevice(device_) != hipSuccess || hipMalloc(&d_ghost_, sizeof(int32_t)) != hipSuccess)) {
        d_ghost_ = nullptr;
        throw Error(URF_ERR_OOM, "BatchDetector: hipMalloc failed");
    }
    if (on && !marker_on_)
        resetRoadMarker();
    marker_on_ = on;
}

void BatchDetector::resetRoadMarker()
{
    if (d_ghost_ && (hipMemsetAsync(d_ghost_, 0, sizeof(int32_t), (hipStream_t)stream_) != hipSuccess))
        throw Error(URF_ERR_HIP, "BatchDetector: hipMemsetAsync failed");
}

/* The MarkerArrays of the S messages just classified (the context's last call): marker points and strips on the device, chained
 * through d_ghost_, one copy back of the counts, records and strip points. */
void BatchDetector::buildMarkers(size_t S)
{
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_pts = al(S * URF_MARKER_MAX_POINTS * 4 * sizeof(float)), b_cnt = al(S * sizeof(uint32_t)), b_n = al(3 * S * sizeof(uint32_t)),
                 b_strips = al(S * URF_MARKER_MAX_STRIPS * sizeof(urf_marker_strip)), b_xyz = al(3 * S * URF_MARKER_MAX_STRIP_POINTS * sizeof(float));
    uint8_t* base = (uint8_t*)grow(d_marker_, d_marker_cap_, b_pts + b_cnt + b_n + b_strips + b_xyz);
    float* d_pts = (float*)base;
    uint32_t* d_cnt = (uint32_t*)(base + b_pts);
    uint8_t* d_out = base + b_pts + b_cnt;
    check(urf_marker_points_batch(ctx_, d_pts, d_cnt), "urf_marker_points_batch");
    check(urf_marker_strips_batch(ctx_, &marker_params_, d_pts, d_cnt, (uint32_t)S, 1, (int32_t*)d_ghost_, (urf_marker_strip*)(d_out + b_n),
                                  (float*)(d_out + b_n + b_strips), (uint32_t*)d_out),
          "urf_marker_strips_batch");
    h_marker_.resize(b_n + b_strips + b_xyz);
    hipStream_t st = (hipStream_t)stream_;
    if (hipMemcpyAsync(h_marker_.data(), d_out, h_marker_.size(), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        throw Error(URF_ERR_HIP, "BatchDetector: read-back failed");
    const uint32_t* n = (const uint32_t*)h_marker_.data();
    const urf_marker_strip* strips = (const urf_marker_strip*)(h_marker_.data() + b_n);
    const float* xyz = (const float*)(h_marker_.data() + b_n + b_strips);
    for (size_t i = 0; i < S; i++) {
        if (n[3 * i + 1] > URF_MARKER_MAX_STRIPS || n[3 * i + 2] > URF_MARKER_MAX_STRIP_POINTS)
            throw Error(URF_ERR_HIP, "BatchDetector: marker counts out of range");
        marker_published_[i] = n[3 * i] != 0;
        if (marker_published_[i])
            toMarkerArray(strips + i * URF_MARKER_MAX_STRIPS, n[3 * i + 1], xyz + 3 * i * URF_MARKER_MAX_STRIP_POINTS, fixed_frame_, markers_[i]);
    }
}

void* BatchDetector::grow(void*& p, size_t& cap, size_t bytes)
{
    if (bytes > cap) {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            throw Error(URF_ERR_OOM, "BatchDetector: hipMalloc failed");
        }
        cap = want;
    }
    return p;
}

void BatchDetector::setDenseRealign(uint32_t max_firings, const std::vector<uint8_t>& slot_of_ring)
{
    if (slot_of_ring.size() > 256)
        throw Error(URF_ERR_INVALID_ARG, "BatchDetector: a slot map holds at most 256 rings");
    check(urf_set_dense_slots(ctx_, slot_of_ring.empty() ? nullptr : slot_of_ring.data(), (uint32_t)slot_of_ring.size()), "urf_set_dense_slots");
    dense_firings_ = max_firings;
}

void BatchDetector::setDenseElevations(const std::vector<float>& elev_deg)
{
    check(urf_set_dense_elevations(ctx_, elev_deg.empty() ? nullptr : elev_deg.data(), (uint32_t)elev_deg.size()), "urf_set_dense_elevations");
    dense_elev_n_ = elev_deg.size();
}

/* the `ring` field of a record layout: UINT8 or UINT16, count 1, inside the record; bytes = 0: none */
static void ringField(const PointCloud2& m, uint32_t& off, uint32_t& bytes)
{
    off = bytes = 0;
    for (const PointField& f : m.fields)
        if (f.name == "ring" && f.count == 1 && (f.datatype == PointField::UINT8 || f.datatype == PointField::UINT16)) {
            const uint32_t b = f.datatype == PointField::UINT8 ? 1u : 2u;
            if ((uint64_t)f.offset + b <= m.point_step) {
                off = f.offset;
                bytes = b;
            }
            return;
        }
}

size_t BatchDetector::filtered(const std::vector<PointCloud2>& msgs)
{
    const size_t S = msgs.size();
    dense_aligned_ = 0;
    infos_.assign(S, urf_scan_info{});
    clouds_.resize(4 * S);
    markers_.resize(S);
    marker_published_.assign(S, 0);   /* (messages that publish nothing leave the ghost count alone: nothing to do for a batch of them) */
    for (size_t i = 0; i < S; i++)
        for (int k = 0; k < 4; k++) {
            clouds_[4 * i + k].header = msgs[i].header;   /* lidar_segmentation.cpp:612-615 */
            clouds_[4 * i + k].points.clear();
        }
    if (S == 0)
        return 0;
    if (S > max_batch_)
        throw Error(URF_ERR_CAPACITY, "BatchDetector: more messages than max_batch");
    /* one record layout for the whole batch, fields by name as Detector::resolve (pcl::fromROSMsg) finds them */
    uint32_t off[3] = { 0, 0, 0 };
    int64_t oi = -1;
    std::vector<uint32_t> offsets(S + 1, 0);
    uint32_t max_len = 0;
    uint64_t total = 0;
    for (size_t i = 0; i < S; i++) {
        uint32_t o[3] = { 0, 0, 0 };
        int64_t oii = -1;
        uint64_t n = 0;
        Detector::resolve(msgs[i], o, oii, n);
        if (i == 0) {
            std::memcpy(off, o, sizeof(off));
            oi = oii;
        } else if (std::memcmp(off, o, sizeof(off)) != 0 || oi != oii || msgs[i].point_step != msgs[0].point_step) {
            throw Error(URF_ERR_INVALID_ARG, "BatchDetector: the messages of a batch must share their record layout");
        }
        if (n > max_points_)
            throw Error(URF_ERR_CAPACITY, "BatchDetector: a message holds more than max_points points");
        total += n;
        max_len = n > max_len ? (uint32_t)n : max_len;
        offsets[i + 1] = (uint32_t)total;
    }
    if (total > (uint64_t)max_points_ * max_batch_)
        throw Error(URF_ERR_CAPACITY, "BatchDetector: more points than max_points * max_batch");
    const uint32_t step = msgs[0].point_step;
    if (total == 0) {   /* nothing but empty messages: what Detector answers for each */
        for (auto& in : infos_)
            in.status = URF_TOO_FEW_POINTS;
        return 0;
    }
    /* the messages back to back, one upload */
    h_data_.resize((size_t)total * step);
    for (size_t i = 0; i < S; i++)
        if (offsets[i + 1] > offsets[i])
            std::memcpy(h_data_.data() + (size_t)offsets[i] * step, msgs[i].data.data(), (size_t)(offsets[i + 1] - offsets[i]) * step);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_off = al((S + 1) * sizeof(uint32_t)), b_lab = al((size_t)total), b_info = al(S * sizeof(urf_scan_info)),
                 b_cnt = al(4 * S * sizeof(uint32_t)), b_offs = al(4 * S * sizeof(uint64_t));
    uint8_t* small = (uint8_t*)grow(d_small_, d_small_cap_, b_off + b_lab + b_info + b_cnt + b_offs);
    uint32_t* d_offsets = (uint32_t*)small;
    uint8_t* d_labels = small + b_off;
    urf_scan_info* d_info = (urf_scan_info*)(small + b_off + b_lab);
    uint32_t* d_counts = (uint32_t*)(small + b_off + b_lab + b_info);
    uint64_t* d_roffs = (uint64_t*)(small + b_off + b_lab + b_info + b_cnt);
    uint8_t* d_data = (uint8_t*)grow(d_data_, d_data_cap_, h_data_.size());
    const uint64_t capacity = 3ull * S * max_len;
    urf_point_xyzi* d_rec = (urf_point_xyzi*)grow(d_records_, d_records_cap_, (size_t)capacity * sizeof(urf_point_xyzi));
    hipStream_t st = (hipStream_t)stream_;
    if (hipMemcpyAsync(d_data, h_data_.data(), h_data_.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_offsets, offsets.data(), (S + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess)
        throw Error(URF_ERR_HIP, "BatchDetector: upload failed");
    /* setDenseRealign: every message carries the same `ring` field (or none does: setDenseElevations), input order (or setDenseOutputs: the reference order comes back in the
     * messages' indices), and the sensor's padded sweep fits the context */
    uint32_t ring_off = 0, ring_bytes = 0;
    bool by_elevation = false;   /* setDenseElevations: no message carries the field, and the table fits the parameters */
    if (dense_firings_ != 0 && (!reference_order_ || dense_outputs_)) {
        ringField(msgs[0], ring_off, ring_bytes);
        by_elevation = ring_bytes == 0 && dense_elev_n_ != 0 && dense_elev_n_ == (size_t)params().channels;
        for (size_t i = 1; i < S && (ring_bytes || by_elevation); i++) {
            uint32_t o = 0, b = 0;
            ringField(msgs[i], o, b);
            if (o != ring_off || b != ring_bytes)
                ring_bytes = 0;
            if (b != 0)
                by_elevation = false;
        }
        const uint64_t padded = (uint64_t)dense_firings_ * (uint32_t)params().channels;
        if (padded > max_points_ || max_len > padded) {
            ring_bytes = 0;
            by_elevation = false;
        }
    }
    if (by_elevation) {
        check(urf_classify_batch_pc2_dense_elev(ctx_, d_data, d_offsets, total, max_len, (uint32_t)S, step, off[0], off[1], off[2], dense_firings_,
                                                d_labels, d_info),
              "urf_classify_batch_pc2_dense_elev");
    } else if (ring_bytes) {
        check(urf_classify_batch_pc2_dense(ctx_, d_data, d_offsets, total, max_len, (uint32_t)S, step, off[0], off[1], off[2], ring_off, ring_bytes,
                                           dense_firings_, d_labels, d_info),
              "urf_classify_batch_pc2_dense");
    } else {
        check(urf_classify_batch_pc2_ragged(ctx_, d_data, d_offsets, total, max_len, (uint32_t)S, step, off[0], off[1], off[2], d_labels, d_info),
              "urf_classify_batch_pc2_ragged");
    }
    check(urf_clouds_batch_pc2(ctx_, d_data, step, off[0], off[1], off[2], (int32_t)oi, reference_order_ ? URF_ORDER_REFERENCE : URF_ORDER_INPUT,
                               d_rec, capacity, d_counts, d_roffs),
          "urf_clouds_batch_pc2");
    /* the counts, then exactly the records they add up to */
    std::vector<uint32_t> counts(4 * S);
    std::vector<uint64_t> roffs(4 * S);
    if (hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(roffs.data(), d_roffs, roffs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(infos_.data(), d_info, S * sizeof(urf_scan_info), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        throw Error(URF_ERR_HIP, "BatchDetector: read-back failed");
    const uint64_t n_rec = roffs[4 * S - 1] + counts[4 * S - 1];
    h_records_.resize(n_rec);
    if (n_rec && (hipMemcpyAsync(h_records_.data(), d_rec, n_rec * sizeof(urf_point_xyzi), hipMemcpyDeviceToHost, st) != hipSuccess ||
                  hipStreamSynchronize(st) != hipSuccess))
        throw Error(URF_ERR_HIP, "BatchDetector: read-back failed");
    if (ring_bytes || by_elevation) {
        uint32_t n_aligned = 0;
        check(urf_dense_scans(ctx_, &n_aligned), "urf_dense_scans");
        dense_aligned_ = n_aligned;
    }
    if (marker_on_)
        buildMarkers(S);
    size_t n_pub = 0;
    for (size_t i = 0; i < S; i++) {
        n_pub += infos_[i].status == URF_OK;
        for (int k = 0; k < 4; k++) {
            auto& pts = clouds_[4 * i + k].points;
            pts.resize(counts[4 * i + k]);
            if (!pts.empty())
                std::memcpy((void*)pts.data(), h_records_.data() + roffs[4 * i + k], pts.size() * sizeof(PointXYZI));
        }
    }
    return n_pub;
}

}   // namespace urf
