/*
 * detector.hpp -- C++ host adapter with the shape of the reference's Detector
 * (include/urban_road_filter/data_structures.hpp:110-141), on top of the C ABI.
 *
 *   reference                                        here
 *   ------------------------------------------------ -----------------------------------------
 *   Detector::Detector(ros::NodeHandle*)             urf::Detector::Detector(device, max_points)
 *     subscribe + advertise + beam_init()              urf_create(): scratch + beam_init tables
 *     (lidar_segmentation.cpp:51-65)
 *   paramsCallback(config, level) (main.cpp:4-34)    urf::Detector::setParams(const urf_params&)
 *   void filtered(const pcl::PointCloud<PointXYZI>&) bool filtered(const PointCloud&)
 *     (lidar_segmentation.cpp:95)                      false <=> the reference returns without
 *                                                      publishing (< 30 ROI points, :124-126)
 *   pub_road/pub_high/pub_box/pub_pobroad.publish    road() curb() roi() road_probably()
 *     (lidar_segmentation.cpp:612-621)                 clouds carrying the input header
 *
 * A ROS node keeps its subscriber/publishers and calls this class from its
 * callback; see INTEGRATION.md.  Points keep their intensity (the reference copies whole
 * pcl::PointXYZI records into its output clouds, lidar_segmentation.cpp:238-242, 354-367); the order
 * inside the output clouds is input order, or, after setReferenceOrder(true), exactly the
 * reference's (ring-major, azimuth ascending).
 *
 * Nothing is allocated per sweep once the clouds have reached their working size (the reference
 * allocates channels x piece x 64 B per callback, :207): the sweep goes through the four-slot
 * asynchronous path of the C ABI (urf_classify_pc2_async / _wait), the label bytes are read in place
 * from the slot's pinned result buffer (urf_result_labels), the index scratch of the reference
 * order lives in the object.  submit() / collect() expose the slots: up to URF_MAX_IN_FLIGHT sweeps in
 * flight, so that a node's subscriber callback returns after the submission.
 */
#ifndef URF_DETECTOR_HPP
#define URF_DETECTOR_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "marker.hpp"
#include "urf.h"

namespace urf {

/* layout of pcl::PointXYZI: 32 bytes, x y z at 0/4/8, intensity at 16 */
struct alignas(16) PointXYZI {
    float x = 0, y = 0, z = 0, pad0 = 1.0f;
    float intensity = 0;
    float pad1[3] = { 0, 0, 0 };
};
static_assert(sizeof(PointXYZI) == sizeof(urf_point_xyzi) && offsetof(PointXYZI, x) == offsetof(urf_point_xyzi, x) &&
                  offsetof(PointXYZI, y) == offsetof(urf_point_xyzi, y) && offsetof(PointXYZI, z) == offsetof(urf_point_xyzi, z) &&
                  offsetof(PointXYZI, pad0) == offsetof(urf_point_xyzi, w) &&
                  offsetof(PointXYZI, intensity) == offsetof(urf_point_xyzi, intensity) &&
                  offsetof(PointXYZI, pad1) == offsetof(urf_point_xyzi, pad),
              "urf::PointXYZI and urf_point_xyzi (include/urf.h) must share their layout: the batch clouds are copied as bytes");

struct Header {
    uint32_t seq = 0;
    uint64_t stamp = 0;
    std::string frame_id;
};

struct PointCloud {
    Header header;
    std::vector<PointXYZI> points;
};

/* sensor_msgs/PointField and sensor_msgs/PointCloud2, field for field */
struct PointField {
    enum { INT8 = 1, UINT8 = 2, INT16 = 3, UINT16 = 4, INT32 = 5, UINT32 = 6, FLOAT32 = 7, FLOAT64 = 8 };
    std::string name;
    uint32_t offset = 0;
    uint8_t datatype = 0;
    uint32_t count = 1;
};
struct PointCloud2 {
    Header header;
    uint32_t height = 1, width = 0;
    std::vector<PointField> fields;
    bool is_bigendian = false;
    uint32_t point_step = 0, row_step = 0;
    std::vector<uint8_t> data;
    bool is_dense = false;
};

/* The switches of the fused front end, for both adapters: each setter forwards to the entry point of include/urf.h it is named after and
 * throws Error(code, that entry point's name) when it fails.  All are off by default and opt-in. */
class FrontSwitches {
public:
    /* urf_set_front_outputs: the reference order and road_marker of a sweep or batch that took the fused front end (a row-major organised
     * stream) come from that run as it is, instead of a second one through the general kernels that keeps the context on them: with it,
     * what takes the fused front end keeps taking it with setReferenceOrder(true) / enableRoadMarker(true). */
    void setFrontOutputs(bool on) { set(urf_set_front_outputs, "urf_set_front_outputs", on); }
    /* urf_set_front_lasers128 / urf_set_front_long_sweeps: front modes 2 and 3 also take sweeps of 128 lasers per firing (channels == 128,
     * curbPoints == 5) / of 129..256 tiles of 2048 points (a 128 x 4096 sweep is 256). */
    void setFrontLasers128(bool on) { set(urf_set_front_lasers128, "urf_set_front_lasers128", on); }
    void setFrontLongSweeps(bool on) { set(urf_set_front_long_sweeps, "urf_set_front_long_sweeps", on); }
    /* urf_set_front_curb_points: front mode 3 also takes curbPoints 1..8 with channels == 16 or 32, and with 128 when setFrontLasers128
     * is on (otherwise 64 lasers only). */
    void setFrontCurbPoints(bool on) { set(urf_set_front_curb_points, "urf_set_front_curb_points", on); }
    /* urf_set_front_multi_sector: the fused front end keeps scans whose firings span several star sectors or whose sectors fall inside a
     * tile (real sensors' azimuth offsets, rotation during a firing, the sweep's seam), with the star-shaped search on and curbPoints == 5 ... */
    void setFrontMultiSector(bool on) { set(urf_set_front_multi_sector, "urf_set_front_multi_sector", on); }
    /* urf_set_front_multi_sector_curb_points: ... and, on top of setFrontMultiSector, with every curbPoints 1..8 that front mode 3 (and
     * setFrontCurbPoints) sends through the fused front end.  Decides nothing while setFrontMultiSector is off.  Times: profiles/front_multi_sector_cp_bench.json. */
    void setFrontMultiSectorCurbPoints(bool on) { set(urf_set_front_multi_sector_curb_points, "urf_set_front_multi_sector_curb_points", on); }
    /* urf_set_front_auto: one switch instead of the five above and mode 3 -- with setFrontMode(2) the context turns on what its sweeps need
     * to stay fused, the call's advice at the call, the scans' after a learning pass behind its first few fused calls (at most five).  It
     * only ever adds; frontAuto().applied names what it turned on, and setFrontAuto(false) leaves that as it is. */
    void setFrontAuto(bool on) { set(urf_set_front_auto, "urf_set_front_auto", on); }
    /* urf_set_front_mode: 0 never, 1 (default) large batches of 64-laser sweeps, 2 every call the fused kernels apply to, 3 as 2 and
     * curbPoints 1..8 -- setFrontAuto acts in modes 2 and 3 only. */
    void setFrontMode(int mode)
    {
        const int rc = urf_set_front_mode(ctx_, mode);
        if (rc != URF_OK)
            throw Error(rc, "urf_set_front_mode");
    }
    /* urf_front_auto_query: phase (URF_AUTO_*), the URF_ADVICE_* bits applied / refused / left, the last digest.  Synchronises. */
    urf_front_auto_info frontAuto() const
    {
        urf_front_auto_info info;
        const int rc = urf_front_auto_query(ctx_, &info);
        if (rc != URF_OK)
            throw Error(rc, "urf_front_auto_query");
        return info;
    }

    /* urf_front_explain: why each scan of the last call (Detector: the sweep waited for last; BatchDetector: the messages of the last
     * filtered()) left the fused front end, and which of the setters above keeps it.  layout: 0 firing order, 1 row-major organised.
     * Changes nothing about the calls to come. */
    std::vector<urf_front_why> frontExplain(int layout)
    {
        const int n = urf_front_explain(ctx_, layout, nullptr, 0);   /* (the last call's scans) */
        if (n < 0)
            throw Error(n, "urf_front_explain");
        std::vector<urf_front_why> why((size_t)n);
        const int rc = n ? urf_front_explain(ctx_, layout, why.data(), (uint32_t)n) : URF_OK;
        if (rc != URF_OK)
            throw Error(rc, "urf_front_explain");
        return why;
    }
    /* one English line per bit that is set and per setter the record advises, by its name */
    static std::string describe(const urf_front_why& w)
    {
        static const struct { uint32_t urf_front_why::*word; uint32_t bit; const char* text; } LINES[] = {
            { &urf_front_why::call, URF_WHY_CALL_MODE_OFF, "call: the fused front end is off (urf_set_front_mode 0)" },
            { &urf_front_why::call, URF_WHY_CALL_STOPPED, "call: front mode 1 stopped trying after a whole batch was handed back" },
            { &urf_front_why::call, URF_WHY_CALL_READOUT, "call: a read-out of ring-sorted results turned the context to the general kernels" },
            { &urf_front_why::call, URF_WHY_CALL_CAPTURE, "call: stage capture is on" },
            { &urf_front_why::call, URF_WHY_CALL_LASERS, "call: no fused kernels for this params.channels under the settings" },
            { &urf_front_why::call, URF_WHY_CALL_CURB_POINTS, "call: no fused kernels for this params.curbPoints under the settings" },
            { &urf_front_why::call, URF_WHY_CALL_TILES, "call: the longest scan has more tiles of 2048 points than the settings take" },
            { &urf_front_why::call, URF_WHY_CALL_FEW_SCANS, "call: fewer scans than front mode 1 takes" },
            { &urf_front_why::call, URF_WHY_CALL_CALLBACK, "call: a sweep of the callback path in firing order" },
            { &urf_front_why::scan, URF_WHY_SCAN_LANE_TWO_RINGS, "scan: a laser slot meets two rings" },
            { &urf_front_why::scan, URF_WHY_SCAN_RING_TWO_LANES, "scan: a ring is fed by two laser slots" },
            { &urf_front_why::scan, URF_WHY_SCAN_AXIS, "scan: a ring point lies on the sensor's axis" },
            { &urf_front_why::scan, URF_WHY_SCAN_RANGE, "scan: a planar range outside [2^-45, 2^63]" },
            { &urf_front_why::scan, URF_WHY_SCAN_ROWS_LENGTH, "scan: row-major, but its length is not params.channels whole rows" },
            { &urf_front_why::scan, URF_WHY_SCAN_MULTI_SECTOR, "scan: a firing spans several star sectors" },
            { &urf_front_why::scan, URF_WHY_SCAN_SECTORS_FALL, "scan: the star sectors fall inside a tile" },
            { &urf_front_why::scan, URF_WHY_SCAN_CANDIDATES, "scan: the candidate list was full" },
            { &urf_front_why::scan, URF_WHY_SCAN_ROWS_SIGHTING, "scan: row-major, and this call could only sight the layout" },
            { &urf_front_why::scan, URF_WHY_SCAN_OTHER, "scan: handed back for no rule known here: a repaired speculation (look-ahead table, ring-count hint, the rows' table), which leaves no word behind" },
            { &urf_front_why::advice, URF_ADVICE_MODE_2, "advice: urf_set_front_mode(ctx, 2)" },
            { &urf_front_why::advice, URF_ADVICE_MODE_3, "advice: urf_set_front_mode(ctx, 3)" },
            { &urf_front_why::advice, URF_ADVICE_LASERS128, "advice: urf_set_front_lasers128(ctx, 1)" },
            { &urf_front_why::advice, URF_ADVICE_LONG_SWEEPS, "advice: urf_set_front_long_sweeps(ctx, 1)" },
            { &urf_front_why::advice, URF_ADVICE_CURB_POINTS, "advice: urf_set_front_curb_points(ctx, 1)" },
            { &urf_front_why::advice, URF_ADVICE_MULTI_SECTOR, "advice: urf_set_front_multi_sector(ctx, 1)" },
            { &urf_front_why::advice, URF_ADVICE_MULTI_SECTOR_CP, "advice: urf_set_front_multi_sector_curb_points(ctx, 1)" },
            { &urf_front_why::advice, URF_ADVICE_FRONT_OUTPUTS, "advice: urf_set_front_outputs(ctx, 1), so that read-outs leave the context fused (callback path: urf_set_sweep_outputs / Detector::setSweepOutputs, whose sweeps need no read-out; setSweepResultsDirect packs what they bring along)" },
            { &urf_front_why::advice, URF_ADVICE_RESET, "advice: call urf_set_front_mode again: it forgets the hand-backs and the read-out" },
            { &urf_front_why::advice, URF_ADVICE_CAPTURE_OFF, "advice: urf_enable_stage_capture(ctx, 0)" },
            { &urf_front_why::advice, URF_ADVICE_BATCH, "advice: classify the sweeps with a batch call (urf_classify_batch_*)" },
            { &urf_front_why::advice, URF_ADVICE_NEVER, "advice: no setting helps; check params.channels and params.interval against the sensor" },
            { &urf_front_why::advice, URF_ADVICE_CAPACITY, "advice: create the context for more points per scan (urf_create: max_points), its candidate list grows with them" },
            { &urf_front_why::advice, URF_ADVICE_CALL_AGAIN, "advice: make the call again: the next one does without what this one tried first" },
        };
        std::string text;
        for (const auto& l : LINES)
            if (w.*(l.word) & l.bit)
                text += std::string(l.text) + "\n";
        return text;
    }

protected:
    urf_ctx* ctx_ = nullptr;
    void set(int (*entry)(urf_ctx*, int), const char* name, bool on)
    {
        const int rc = entry(ctx_, on ? 1 : 0);
        if (rc != URF_OK)
            throw Error(rc, name);
    }
};

class Detector : public FrontSwitches {
public:
    explicit Detector(int device = 0, uint32_t max_points = 1u << 20);
    ~Detector();
    Detector(const Detector&) = delete;
    Detector& operator=(const Detector&) = delete;

    /* Emit road / curb / road_probably in the reference's own order (ring by ring, ascending
     * azimuth inside a ring -- lidar_segmentation.cpp:289-291, 354-367) instead of input order.
     * Costs one extra per-ring sort on the GPU; roi is in input order either way. */
    void setReferenceOrder(bool on)
    {
        applySweepOutputs(sweep_outputs_, marker_on_, on);   /* (throws before anything changes) */
        reference_order_ = on;
    }
    /* Also build the "road_marker" MarkerArray (lidar_segmentation.cpp:295-351, 369-602, topic :59,601);
     * fixedFrame = params::fixedFrame (cfg:10).  Off by default: the polygon is a visualisation product. */
    void enableRoadMarker(bool on, const std::string& fixed_frame = "left_os1/os1_lidar")
    {
        applySweepOutputs(sweep_outputs_, on, reference_order_);
        marker_on_ = on;
        marker_.setFixedFrame(fixed_frame);
    }
    /* urf_set_sweep_outputs: with it on, the marker points (enableRoadMarker) and the index lists of the reference order
     * (setReferenceOrder) are produced by the sweep's own launch sequence and travel with its ticket -- collect() reads them from the
     * ticket's result buffers instead of calling urf_marker_points / urf_ordered_indices, which wait for every sweep in flight and need
     * one scratch row per sweep in flight.  With submit() / collect() and several sweeps in flight this keeps the pipelining; the clouds
     * and the MarkerArray are the same byte for byte.  Off (default): the two synchronous calls, as before.  Like the two setters
     * above it is callable between sweeps only: with a sweep in flight it throws Error(URF_ERR_BUSY). */
    void setSweepOutputs(bool on)
    {
        applySweepOutputs(on, marker_on_, reference_order_);
        sweep_outputs_ = on;
    }
    /* urf_set_sweep_results_direct: on top of setSweepOutputs, the kernels of a sweep's sequence store marker points, counts and the lists
     * themselves into mapped pinned memory of the sweep's slot, the lists back to back, instead of three copied arrays of the sweep's
     * length; collect() reads either (urf_result_*), clouds and MarkerArray are the same byte for byte.  Off by default; decides nothing
     * while setSweepOutputs is off.  Between sweeps only: with a sweep in flight it throws Error(URF_ERR_BUSY). */
    void setSweepResultsDirect(bool on);
    /* urf_set_sweep_quantum: for streams whose messages differ in length (velodyne_pointcloud's default mode, any is_dense cloud).  A
     * sweep runs as the next multiple of `points` points (a multiple of 2048, at most max_points), NaN behind its own, so that one
     * captured launch sequence per padded length is replayed instead of a new one per message; clouds, labels and MarkerArray are the
     * same byte for byte.  0 (default): off.  Between sweeps only: with a sweep in flight it throws Error(URF_ERR_BUSY). */
    void setSweepQuantum(uint32_t points);
    void setMarkerParams(const urf_marker_params& p) { marker_.setParams(p); }
    /* nullptr when the reference would not publish a MarkerArray for the last sweep */
    const MarkerArray* road_marker() const { return marker_published_ ? &markers_ : nullptr; }

    /* main.cpp:4-34 paramsCallback: callable between scans */
    void setParams(const urf_params& p);
    urf_params params() const;

    /* lidar_segmentation.cpp:95 Detector::filtered.  Returns false when nothing is published. */
    bool filtered(const PointCloud& cloud);
    /* The same for a raw sensor_msgs/PointCloud2 payload: data, point_step, the byte offsets of the
     * x / y / z FLOAT32 fields and (optional, -1 = the message has none) of the FLOAT32 intensity field.
     * The output clouds carry x, y, z and that intensity (0 without the field: what pcl::fromROSMsg leaves
     * in a pcl::PointXYZI whose field the message lacks). */
    bool filtered(const uint8_t* data, uint32_t n_points, uint32_t point_step,
                  uint32_t off_x, uint32_t off_y, uint32_t off_z, const Header& header = Header(),
                  int64_t off_intensity = -1);

    /* The wire message itself: resolves the x / y / z and intensity FLOAT32 fields by name, as
     * pcl::fromROSMsg does for pcl::PointXYZI (every other field is ignored), and classifies
     * width*height points. */
    bool filtered(const PointCloud2& msg);

    /* The same in two halves, up to URF_MAX_IN_FLIGHT sweeps in flight: submit() returns as soon as the
     * sweep is on its way to the device, collect() blocks until it is done and fills road() ... labels().
     * Tickets must be collected in the order they were submitted; the message (cloud.points / data /
     * msg.data) must stay alive and unchanged until its ticket has been collected -- the output clouds are
     * built from it.  A submission while URF_MAX_IN_FLIGHT sweeps are in flight throws Error(URF_ERR_BUSY). */
    uint32_t submit(const PointCloud& cloud);
    uint32_t submit(const uint8_t* data, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                    uint32_t off_z, const Header& header = Header(), int64_t off_intensity = -1);
    uint32_t submit(const PointCloud2& msg);
    bool collect(uint32_t ticket);

    const PointCloud& road() const { return road_; }                    /* topic "road" */
    const PointCloud& curb() const { return curb_; }                    /* topic "curb" */
    const PointCloud& roi() const { return roi_; }                      /* topic "roi" */
    const PointCloud& road_probably() const { return road_probably_; }  /* topic "road_probably" */
    /* one urf.h label byte per input point of the sweep collected last: n_labels() bytes in the library's
     * pinned result buffer, valid until URF_MAX_IN_FLIGHT further sweeps have been submitted */
    const uint8_t* labels() const { return labels_; }
    uint32_t n_labels() const { return n_labels_; }
    const urf_scan_info& info() const { return info_; }

private:
    struct Pending {
        const uint8_t* data = nullptr;
        uint32_t n = 0, step = 0, ox = 0, oy = 0, oz = 0, ticket = 0;
        int64_t oi = -1;
        Header header;
        bool used = false;
    };
    void check(int rc, const char* what) const;
    void split(const Pending& m);
    static void resolve(const PointCloud2& msg, uint32_t off[3], int64_t& off_intensity, uint64_t& n);
    friend class BatchDetector;
    void applySweepOutputs(bool sweep, bool marker, bool order);   /* urf_set_sweep_outputs with the bits the three settings add up to */
    bool reference_order_ = false;
    bool marker_on_ = false, marker_published_ = false;
    bool sweep_outputs_ = false;
    uint32_t sweep_bits_ = 0;   /* what the context has been told (0: never asked for, nothing allocated) */
    MarkerBuilder marker_;
    MarkerArray markers_;
    Pending pending_[URF_MAX_IN_FLIGHT];
    const uint8_t* labels_ = nullptr;
    uint32_t n_labels_ = 0;
    urf_scan_info info_{};
    PointCloud road_, curb_, roi_, road_probably_;
    std::vector<uint32_t> ord_;   /* 3 x max_points: the index lists of the reference order (sized once) */
    uint32_t max_points_ = 0;
};

/* The batch twin of Detector::filtered(const PointCloud2&), for recorded drives: a vector of wire messages -- of any lengths
 * (drivers that drop non-returns publish variable-length clouds), all with the same record layout -- goes to the device in
 * one copy, through urf_classify_batch_pc2_ragged and urf_clouds_batch_pc2, and the four clouds of every message come back
 * in one copy.  road(i) ... road_probably(i) equal what Detector::filtered gives for message i on its own: the same points
 * in the same order (input order, or the reference's after setReferenceOrder(true)), the same header.  Records carry
 * x / y / z / intensity bit for bit with pcl::PointXYZI's w = 1 and zero padding (what pcl::fromROSMsg leaves; Detector
 * copies a pcl::PointXYZI-layout message's padding bytes as they are, which a message from pcl::toROSMsg holds the same way).
 * One context of max_batch scans of up to max_points points: a call with more messages, or a longer one, throws
 * Error(URF_ERR_CAPACITY).
 * road_marker (enableRoadMarker): the messages of one filtered() call are consecutive sweeps of one sensor, and the ghost count
 * -- all the reference keeps from sweep to sweep -- stays in a device word between calls, so a drive cut into batches of any
 * sizes gives the MarkerArrays Detector gives for the same messages one by one.  Marker points and line strips are built on the
 * device (urf_marker_points_batch -> urf_marker_strips_batch) and come back in one copy; with the marker off, filtered()
 * launches nothing for it. */
class BatchDetector : public FrontSwitches {
public:
    BatchDetector(int device = 0, uint32_t max_points = 1u << 20, uint32_t max_batch = 64);
    ~BatchDetector();
    BatchDetector(const BatchDetector&) = delete;
    BatchDetector& operator=(const BatchDetector&) = delete;

    void setParams(const urf_params& p);
    urf_params params() const;
    void setReferenceOrder(bool on) { reference_order_ = on; }
    /* Dense messages (the driver dropped the non-returns) with a field named "ring" (UINT8 or UINT16, count 1) are put back into firing
     * slots on the device and classified as organised sweeps (urf_classify_batch_pc2_dense, include/urf.h): max_firings = the sensor's
     * firings per revolution, slot_of_ring[ring] = the laser's position inside a firing (empty: the ring is the position).  Same clouds,
     * headers and road_marker either way; off by default, max_firings == 0 turns it off.  Messages without such a field (but see
     * setDenseElevations), the reference order (setReferenceOrder) while setDenseOutputs is off, and a sensor whose max_firings *
     * channels sweep does not fit max_points keep the ragged call. */
    void setDenseRealign(uint32_t max_firings, const std::vector<uint8_t>& slot_of_ring = {});
    /* urf_set_dense_elevations: elev_deg[l] = the elevation in degrees of the laser in slot l of a firing (the sensor's datasheet).  With
     * setDenseRealign on, messages WITHOUT a `ring` field (pcl::PointXYZI, what the reference subscribes to) then take
     * urf_classify_batch_pc2_dense_elev -- the ids derived from the points' elevation on the device -- when the table's size is the
     * parameters' channels; otherwise, and without this call, they keep the ragged call.  Messages with the field are not affected.  An
     * empty vector clears the table. */
    void setDenseElevations(const std::vector<float>& elev_deg);
    /* urf_set_dense_outputs: the reference order after a dense call, in the messages' own indices.  On, setReferenceOrder(true) no longer
     * keeps filtered() off the dense call: same clouds, in the reference's order.  Off (default): filtered() chooses as above. */
    void setDenseOutputs(bool on)
    {
        set(urf_set_dense_outputs, "urf_set_dense_outputs", on);
        dense_outputs_ = on;
    }
    /* messages of the last filtered() call that were put back into firing slots (0 when it took the ragged call), in either order */
    size_t denseAligned() const { return dense_aligned_; }

    /* As Detector's: also build "road_marker" for every message (off by default; the polygon parameters start from
     * urf_default_marker_params, as Detector's do).  Switching it on starts a new drive. */
    void enableRoadMarker(bool on, const std::string& fixed_frame = "left_os1/os1_lidar");
    void setMarkerParams(const urf_marker_params& p) { marker_params_ = p; }
    /* forget the previous sweep's strips (a new drive): the next publishing message emits no DELETE markers */
    void resetRoadMarker();
    /* nullptr when the reference would not publish a MarkerArray for message i of the last filtered() call */
    const MarkerArray* road_marker(size_t i) const { return marker_published_.at(i) ? &markers_[i] : nullptr; }

    /* Classifies every message; returns how many of them publish (the others: < 30 ROI points, or empty). */
    size_t filtered(const std::vector<PointCloud2>& msgs);

    size_t size() const { return infos_.size(); }
    const PointCloud& road(size_t i) const { return clouds_.at(4 * i + 0); }
    const PointCloud& curb(size_t i) const { return clouds_.at(4 * i + 1); }
    const PointCloud& roi(size_t i) const { return clouds_.at(4 * i + 2); }
    const PointCloud& road_probably(size_t i) const { return clouds_.at(4 * i + 3); }
    const urf_scan_info& info(size_t i) const { return infos_.at(i); }
    bool published(size_t i) const { return infos_.at(i).status == URF_OK; }

private:
    void check(int rc, const char* what) const;
    void* grow(void*& p, size_t& cap, size_t bytes);
    void* stream_ = nullptr;
    uint32_t max_points_ = 0, max_batch_ = 0;
    bool reference_order_ = false;
    uint32_t dense_firings_ = 0;   /* setDenseRealign */
    size_t dense_elev_n_ = 0;      /* setDenseElevations */
    bool dense_outputs_ = false;   /* setDenseOutputs */
    size_t dense_aligned_ = 0;
    /* device buffers (grown on demand) */
    void* d_data_ = nullptr;
    size_t d_data_cap_ = 0;
    void* d_records_ = nullptr;
    size_t d_records_cap_ = 0;
    void* d_small_ = nullptr;    /* offsets, labels, infos, counts, record offsets */
    size_t d_small_cap_ = 0;
    std::vector<uint8_t> h_data_;
    std::vector<PointXYZI> h_records_;
    std::vector<urf_scan_info> infos_;
    std::vector<PointCloud> clouds_;   /* 4 per message: road, curb, roi, road_probably */
    /* road_marker */
    void buildMarkers(size_t S);
    int device_ = 0;
    bool marker_on_ = false;
    std::string fixed_frame_;
    urf_marker_params marker_params_;
    void* d_ghost_ = nullptr;    /* int32_t: the ghost count, from call to call */
    void* d_marker_ = nullptr;   /* marker points and counts, then (one read-back) d_n, strips, strip points */
    size_t d_marker_cap_ = 0;
    std::vector<uint8_t> h_marker_;
    std::vector<MarkerArray> markers_;
    std::vector<char> marker_published_;
};

}   // namespace urf
#endif
