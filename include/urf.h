/*
 * urf.h -- C ABI of the MI355X-native urban_road_filter hot path.
 *
 * Drop-in boundary.  The reference processes every LiDAR
 * sweep inside one C++ callback,
 *     void Detector::filtered(const pcl::PointCloud<pcl::PointXYZI>& cloud)
 *         include/urban_road_filter/data_structures.hpp:118
 *         src/lidar_segmentation.cpp:95-622
 * fed by a sensor_msgs/PointCloud2 subscription (src/lidar_segmentation.cpp:53)
 * and answering with the clouds "road", "curb", "roi", "road_probably"
 * (src/lidar_segmentation.cpp:55-58, 354-367, 605-608, 618-621).
 *
 * This library replaces the geometric classification in the middle
 * (lidar_segmentation.cpp:100-293,353-367,605-608 + star_shaped_search.cpp +
 * x_zero_method.cpp + z_zero_method.cpp + blind_spots.cpp) by hand-written
 * gfx950 HIP kernels.  Points go in as PointCloud2-layout bytes (or as SoA
 * x/y/z device arrays for resident batches); what comes out is ONE BYTE PER
 * INPUT POINT that encodes the reference's per-point result:
 *
 *     bits 0-1  isCurbPoint of the reference (data_structures.hpp:44):
 *               0 = none, 1 = road (blind_spots.cpp:128,168,237,277),
 *               2 = curb (star_shaped_search.cpp:146, x_zero_method.cpp:66,
 *               z_zero_method.cpp:71)
 *     bit 2     point passed the ROI filter, i.e. is in the "roi" cloud
 *               (lidar_segmentation.cpp:106-117, 620)
 *     bit 3     point was assigned to a ring (lidar_segmentation.cpp:226-277);
 *               only such points can appear in "road"/"curb"
 *     bit 4     point lies on sorted ring index 10, i.e. is in the
 *               "road_probably" cloud (lidar_segmentation.cpp:605-608)
 *
 * so   road = {i : (label[i] & 3) == 1},  curb = {i : (label[i] & 3) == 2},
 *      roi  = {i : label[i] & 4},  road_probably = {i : label[i] & 16}.
 * The C++ adapter (urban_road_filter_amd/csrc/detector.hpp) re-materialises
 * the four clouds from these sets.  Set membership is the contract; the order
 * of points inside the reference's published clouds is not.
 *
 * All functions return 0 on success, a negative urf_status on error.  One
 * context owns one device, one HIP stream and all scratch memory; a context is
 * not thread-safe, any number of contexts may coexist (the reference keeps its
 * state in globals and allows one Detector per process).
 */
#ifndef URF_H
#define URF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): URF_MAX_IN_FLIGHT sweeps on the asynchronous path (tickets map to slots modulo it),
 * urf_result_labels() validates its ticket, URF_NUM_KERNELS / kernel names as listed below,
 * urf_enable_stage_capture() takes a mode 0..2, urf_scan_info::n_nan_azimuth is written.
 * 3 (round 4): the test / benchmark hooks (urf_synth_cloud, urf_bench_callback_stream, urf_selftest*,
 * urf_set_debug_flags) left this header and the product library (include/urf_test_hooks.h, liburf_hip_test.so);
 * rings that hold a point with x == y == 0 follow the reference (deviation D5 of earlier versions is gone);
 * urf_read_stage / urf_ordered_indices / urf_marker_points answer URF_ERR_BUSY for a sweep whose scratch row has
 * been resubmitted; urf_callback_path_state reports sequence bits 2 and 3.
 * 4 (round 5): equal planar ranges inside a star sector are ordered as libstdc++'s std::sort orders them
 * (star_shaped_search.cpp:109) and equal azimuths inside a ring as the reference's Lomuto quicksort does
 * (lidar_segmentation.cpp:70-93): "deviation D2" of earlier versions is gone, labels on real sensor data (range ties in
 * every sector) and the published order equal the reference's; urf_callback_path_state reports sequence bit 4.
 * 5 (round 6): urf_set_front_mode / urf_front_scans (the fused front end for batches of organised sweeps: firing order and
 * row-major); the entry points that read ring-sorted intermediate results may run the last batch call again, see there;
 * urf_callback_path_preset.
 * Additions under 5, additive (no existing entry point, struct or value changed): urf_classify_batch_pc2_ragged (ragged
 * PointCloud2 batches), urf_clouds_batch_soa / urf_clouds_batch_pc2 with struct urf_point_xyzi, URF_ORDER_INPUT and
 * URF_ORDER_REFERENCE (the four published clouds of a batch as device-resident records); urf_marker_strips /
 * urf_marker_strips_batch with struct urf_marker_strip, URF_MARKER_MAX_STRIPS, URF_MARKER_MAX_STRIP_POINTS (the line strips of
 * road_marker: one sweep on the host, a batch of sweeps on the device); urf_classify_batch_soa_dense / urf_classify_batch_pc2_dense with
 * urf_set_dense_slots and urf_dense_scans (dense sweeps put back into firing slots by laser id on the device, then classified as
 * organised ones); urf_set_front_curb_points (front mode 3's curbPoints 1..8 at 16, 32 and 128 lasers per firing as well);
 * urf_set_front_multi_sector_curb_points (urf_set_front_multi_sector at curbPoints 1..8 instead of 5 only); urf_set_dense_outputs
 * (the reference-order read-outs after a dense call, in the caller's indices); urf_set_dense_elevations with
 * urf_classify_batch_soa_dense_elev / urf_classify_batch_pc2_dense_elev (the dense calls for clouds without a `ring` field: laser ids
 * derived from the points' elevation on the device); urf_set_sweep_outputs with urf_result_marker_points / urf_result_ordered_indices
 * and URF_SWEEP_OUT_* (a sweep of the callback path brings its marker points and ordered lists along, read per ticket);
 * urf_set_sweep_quantum with urf_callback_path_captures and URF_SWEEP_SEQS (sweeps of varying length on the callback path: padded to a
 * quantum of points, one captured sequence per padded length); urf_set_sweep_results_direct (those results stored by the kernels
 * themselves into mapped pinned memory, the lists packed back to back: no copy of unused words).
 * WHICH std::sort (4 above): the one of libstdc++ as shipped with GCC 5 .. 13 (bits/stl_algo.h: __sort = __introsort_loop with
 * _S_threshold 16, __move_median_to_first on (first + 1, mid, last - 1), __unguarded_partition, depth limit 2 * floor(log2 n),
 * __partial_sort as the fallback, then __final_insertion_sort); tests/test_stdsort.py pins the restatement against the std::sort
 * of the build host and FAILS when they disagree.  A reference built against another standard library (libc++) or a future
 * libstdc++ with another __sort orders equal planar ranges differently, and its labels on tied data then differ from this
 * library's at the points concerned -- nothing at run time can tell. */
#define URF_ABI_VERSION 5

/* ---- label byte --------------------------------------------------------- */
#define URF_LABEL_MASK   0x03u
#define URF_LABEL_NONE   0u
#define URF_LABEL_ROAD   1u
#define URF_LABEL_CURB   2u
#define URF_FLAG_ROI     0x04u
#define URF_FLAG_RING    0x08u
#define URF_FLAG_RING10  0x10u

/* ---- status codes ------------------------------------------------------- */
typedef enum urf_status {
    URF_OK = 0,
    /* per-scan status (positive: not an error) */
    URF_TOO_FEW_POINTS = 1,      /* < 30 ROI points: the reference returns without
                                    publishing (lidar_segmentation.cpp:124-126);
                                    every label of the scan is 0 */
    /* errors */
    URF_ERR_INVALID_ARG = -1,
    URF_ERR_NO_DEVICE = -2,      /* no HIP device / runtime error at create */
    URF_ERR_HIP = -3,            /* HIP runtime failure, see urf_last_error() */
    URF_ERR_CAPACITY = -4,       /* scan or batch larger than urf_create() sizes */
    URF_ERR_OOM = -5,
    URF_ERR_PARAMS = -6,         /* parameter outside the supported range */
    URF_ERR_BUSY = -7            /* every slot of the asynchronous single-scan path is in flight (or the asked-for
                                    result is still being written) */
} urf_status;

/* ---- parameters ----------------------------------------------------------
 * The hot-path subset of the reference's 27 dynamic_reconfigure fields
 * (cfg/LidarFilters.cfg:10-84 -> src/main.cpp:4-34 -> namespace params,
 * data_structures.hpp:66-88) plus its three compile-time globals.  Field names
 * follow namespace params.  Types follow the reference (float/int/bool), so
 * e.g. interval is 0.18f, not 0.18.
 */
typedef struct urf_params {
    uint32_t size;               /* = sizeof(urf_params); ABI versioning */
    int32_t  x_zero_method;      /* cfg:16  bool */
    int32_t  z_zero_method;      /* cfg:17  bool */
    int32_t  star_shaped_method; /* cfg:18  bool */
    int32_t  blind_spots;        /* cfg:19  bool */
    int32_t  xDirection;         /* cfg:27  0 both, 1 +X, 2 -X */
    float    interval;           /* cfg:30  ring-angle tolerance [deg] */
    float    curbHeight;         /* cfg:33  curb_height [m] */
    int32_t  curbPoints;         /* cfg:36  curb_points, 1..30 */
    float    beamZone;           /* cfg:39  [deg] */
    float    min_X, max_X;       /* cfg:42-43 */
    float    min_Y, max_Y;       /* cfg:46-47 */
    float    min_Z, max_Z;       /* cfg:50-51 */
    float    angleFilter1;       /* cfg:54  cylinder_deg_x */
    float    angleFilter2;       /* cfg:57  cylinder_deg_z */
    float    angleFilter3;       /* cfg:60  curb_slope_deg */
    float    kdev_param;         /* cfg:63 */
    float    kdist_param;        /* cfg:66 */
    int32_t  starbeam_filter;    /* cfg:69  bool */
    int32_t  dmin_param;         /* cfg:72 */
    int32_t  channels;           /* lidar_segmentation.cpp:4   (64), 1..128: the ring table's capacity -- set it to the sensor's laser count; 16, 32 and 64
                                  * also state the points per firing to the fused front end (urf_set_front_mode) */
    int32_t  sectors;            /* star_shaped_search.cpp:8   rep = 360 */
    float    beam_width;         /* star_shaped_search.cpp:9   width = 0.2 */
} urf_params;

/* Fills *p with the reference defaults (cfg/LidarFilters.cfg) and the
 * reference's compile-time globals (channels 64, rep 360, width 0.2). */
int urf_default_params(urf_params* p);

/* ---- the live parameter surface ---------------------------------------------
 * One descriptor per gen.add() of cfg/LidarFilters.cfg:10-84 (the node's dynamic_reconfigure
 * interface): the reference's parameter name, type, default and range, the xDirection enum
 * (:22-27), and where the value lives in urf_params / urf_marker_params (`field`, `offset`).
 * fixed_frame / topic_name configure the ROS node, not the classification (URF_PARAM_NODE_ONLY).
 * urf_clamp_params() does what the dynamic_reconfigure server does to a request before
 * paramsCallback (src/main.cpp:4-34) sees it: every value is clamped to [min, max], bools become
 * 0/1; *n_clamped (optional) = number of values it changed.  mp may be NULL.  (urf_set_params still
 * rejects what the kernels cannot run: channels, sectors, curbPoints outside their limits.) */
typedef enum urf_param_type { URF_PARAM_BOOL = 0, URF_PARAM_INT = 1, URF_PARAM_DOUBLE = 2, URF_PARAM_STR = 3 } urf_param_type;
typedef enum urf_param_where { URF_PARAM_IN_PARAMS = 0, URF_PARAM_IN_MARKER_PARAMS = 1, URF_PARAM_NODE_ONLY = 2 } urf_param_where;
typedef struct urf_param_desc {
    const char* cfg_name;    /* name in cfg/LidarFilters.cfg */
    const char* field;       /* member of urf_params / urf_marker_params ("" = node only) */
    int32_t     where;       /* urf_param_where */
    uint32_t    offset;      /* byte offset of the member (float for double_t, int32_t for int_t / bool_t) */
    int32_t     type;        /* urf_param_type (the cfg's type) */
    double      def, min, max;
    const char* def_str;     /* default of a str_t, else NULL */
    const char* enum_values; /* "name=value,..." where the cfg defines an enum, else NULL */
    int32_t     cfg_line;    /* line of the gen.add() */
} urf_param_desc;
struct urf_marker_params;
int urf_param_count(void);
const urf_param_desc* urf_param_table(void);
int urf_clamp_params(urf_params* p, struct urf_marker_params* mp, uint32_t* n_clamped);

/* ---- per-scan summary ---------------------------------------------------- */
typedef struct urf_scan_info {
    int32_t  status;     /* URF_OK or URF_TOO_FEW_POINTS */
    uint32_t n_roi;      /* "piece",  lidar_segmentation.cpp:120 */
    uint32_t n_rings;    /* "index",  lidar_segmentation.cpp:139,194 */
    uint32_t n_ring_pts; /* points assigned to a ring */
    uint32_t n_road;     /* size of the "road" cloud */
    uint32_t n_curb;     /* size of the "curb" cloud */
    uint32_t n_ring10;   /* size of "road_probably" */
    uint32_t n_nan_azimuth; /* ring points with x == y == 0 (azimuth NaN): 0 on every real sweep; followed as the
                               reference treats them, see below */
} urf_scan_info;
/* A ring point with x == y == 0 has d = 0 and azimuth asin(0 / 0) = NaN (lidar_segmentation.cpp:245-269).  In the
 * reference that NaN goes through the per-ring Lomuto quicksort (:70-93), where every comparison with it is false: the
 * point ends up at an input-order-dependent place of the sorted ring, and the beam scans of blind_spots.cpp
 * (:107,146,216,255) end there -- forward beams see only what stands in front of the ring's first NaN, backward beams only
 * what stands behind its last one.  Deterministic, hence followed: for such a ring the library runs the reference's
 * quicksort literally (k_nan_rings) and limits the beams accordingly; labels, counters and the published order
 * (urf_ordered_indices) equal the reference's.  (Up to round 3 this was "deviation D5": such a point simply never became
 * road and never cut a beam short.)  n_nan_azimuth counts these points (0 on every real sweep: a return at the sensor's
 * own axis).  One residue: two points of such a ring with bit-identical azimuths on either side of a NaN's place are told
 * apart by position in the reference and by value here.
 * COST: the quicksort is the reference's own -- Lomuto, pivot = last element, O(n^2) on the nearly sorted rings of an
 * organised sweep (56 % of the reference's CPU time goes there) -- run by ONE wave per such ring: about 1 ms for a ring of
 * 2 048 points, several ms for a ring beyond 6 144 points (sorted in global memory), against ~0.13 ms for the whole sweep
 * otherwise; on the callback path the first such sweep is additionally run twice (urf_callback_path_state).  A region of
 * interest that excludes the sensor's own axis (the reference's "x + y + z != 0" filter already drops (0, 0, 0) filler
 * points) never gets here. */

typedef struct urf_ctx urf_ctx;

/* ---- lifetime ------------------------------------------------------------
 * Replaces Detector::Detector (lidar_segmentation.cpp:51-65): allocates every
 * scratch buffer once (the reference allocates channels x piece x 64 B per
 * scan, lidar_segmentation.cpp:207) and runs beam_init()
 * (star_shaped_search.cpp:32-66).  max_points bounds the points of one scan,
 * max_batch the scans of one batch call. */
int urf_create(urf_ctx** ctx, int device_id, uint32_t max_points, uint32_t max_batch);
int urf_destroy(urf_ctx* ctx);

/* Replaces paramsCallback (src/main.cpp:4-34): may be called between scans.
 * THE PARAMETER BOX.  Every value the node's dynamic_reconfigure server can deliver -- each row of urf_param_table() anywhere in
 * its [min, max], one at its end or all of them at theirs (interval 0.01 and 10, curbHeight 0.5, curbPoints 1 and 30, beamZone 10
 * and 100, angleFilter1 / 2 / 3 at 0 and 180, a region of interest that is empty or inverted: URF_TOO_FEW_POINTS for every scan) --
 * is followed bit for bit by every entry point: labels, summaries, published order and marker points are the reference's
 * (tests/test_gpu_param_edges.py against oracle B, tests/test_param_edges_cpu.py oracle B against the reference's own sources).
 * Outside the box the reference stays defined, and urf_set_params takes and follows in the same way: interval 0, above 10 and
 * +Inf (every point on one ring); beamZone anywhere in (0, 360]; any angleFilter1 / 2 / 3, negative, above 180 and NaN included;
 * any curbHeight, kdev_param, kdist_param (0, negative, NaN) and dmin_param; region-of-interest bounds beyond +-200, infinite or
 * NaN (a NaN bound keeps no point); any beam_width.  It refuses, with URF_ERR_PARAMS and the parameters in force unchanged:
 * channels outside 1..128, sectors outside 1..1022, curbPoints outside 1..30, xDirection outside 0..2,
 * beamZone <= 0, above 360 or NaN, interval negative or NaN.
 * Which kernels run does depend on the values (urf_set_front_mode below: curbPoints 9..30 and an interval that merges two lasers
 * into one ring keep the general kernels); the results do not. */
int urf_set_params(urf_ctx* ctx, const urf_params* p);
int urf_get_params(const urf_ctx* ctx, urf_params* p);

/* Run on a caller-owned hipStream_t (e.g. the framework's current stream);
 * NULL restores the context's own stream. */
int urf_set_stream(urf_ctx* ctx, void* hip_stream);
int urf_synchronize(urf_ctx* ctx);

/* ---- single scan, host buffers, PointCloud2 layout ------------------------
 * Replaces the body of Detector::filtered for one sensor_msgs/PointCloud2:
 * `data` holds n_points records of point_step bytes; x/y/z are little-endian
 * FLOAT32 at byte offsets off_x/off_y/off_z (pcl::fromROSMsg resolves the
 * fields by name; every other field is ignored, as pcl::PointXYZI ignores
 * them).  labels_out (host, n_points bytes) receives the label bytes, *info
 * (optional) the summary.  Synchronous.  Returns URF_OK or an error; the
 * "too few points" condition is reported in info->status. */
int urf_classify_pc2(urf_ctx* ctx, const uint8_t* data, uint32_t n_points,
                     uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                     uint8_t* labels_out, urf_scan_info* info);

/* The same, asynchronously: the message's x / y / z are gathered into pinned memory (three planes: 12 bytes
 * per point cross PCIe whatever the point_step) and sent to the device, classified by ONE graph launch (the
 * kernel sequence of a sweep of this shape is captured once and replayed), and the labels come back to pinned
 * memory.  URF_MAX_IN_FLIGHT sweeps may be in flight; with a context created for max_batch >= 2 they are spread
 * over min(max_batch, URF_MAX_IN_FLIGHT) scratch rows, each with its own stream (copy in, kernels, copy out), so
 * that the copies and kernels of different sweeps overlap -- create the context with max_batch >= 4 for the
 * callback path:
 *     urf_classify_pc2_async(ctx, msg_a, ..., &ta);
 *     urf_classify_pc2_async(ctx, msg_b, ..., &tb);      // ... the fifth in a row returns URF_ERR_BUSY
 *     urf_classify_pc2_wait(ctx, ta, labels_a, &info_a);  // blocks until sweep a is done
 * Sweeps must be waited for in the order they were submitted if the results are to be looked at with
 * urf_read_stage / urf_ordered_indices / urf_marker_points (those see the sweep waited for last).
 * SHARED ROWS: with max_batch < URF_MAX_IN_FLIGHT the slots share min(max_batch, URF_MAX_IN_FLIGHT) scratch rows
 * (slot i uses row i modulo that number; slots on one row are serialised).  Labels and summary of every sweep are
 * right whatever the sharing -- each slot has result buffers of its own --, but the three entry points just named
 * read the sweep's ROW: once a later sweep has been submitted on that row they return URF_ERR_BUSY instead of mixing
 * two sweeps' intermediate results.  Create the context with max_batch >= the number of sweeps kept in flight, or
 * read a sweep's intermediate results before submitting on its row again.
 * Every other entry point of the context that touches its scratch memory (the batch calls, the three
 * just named, urf_compact_indices*) is ordered behind the sweeps still in flight; urf_synchronize()
 * waits for them as well.
 * labels_out may be NULL: urf_result_labels() then gives read access to the pinned result buffer of a
 * ticket that has been waited for, valid until the ticket's slot is used again (URF_MAX_IN_FLIGHT
 * submissions later); a ticket never issued or overtaken is refused with URF_ERR_INVALID_ARG, one
 * still in flight with URF_ERR_BUSY.  A producer that can fill a
 * buffer of the library's choosing (a driver, a deserialiser) saves the staging copy: it asks for
 * the pinned input buffer of the NEXT submission with urf_pinned_input() (URF_ERR_BUSY while that
 * slot is still in flight), writes the message there and passes that very pointer as `data` (a message
 * that starts inside that buffer but is not exactly it, or is longer than the size asked for, is
 * refused with URF_ERR_INVALID_ARG).  Reference: the subscriber callback, lidar_segmentation.cpp:53,95-100, and
 * the publishers, :612-621. */
#define URF_MAX_IN_FLIGHT 4
int urf_classify_pc2_async(urf_ctx* ctx, const uint8_t* data, uint32_t n_points,
                           uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                           uint32_t* ticket);
int urf_classify_pc2_wait(urf_ctx* ctx, uint32_t ticket, uint8_t* labels_out, urf_scan_info* info);
int urf_result_labels(urf_ctx* ctx, uint32_t ticket, const uint8_t** labels);
int urf_pinned_input(urf_ctx* ctx, size_t bytes, uint8_t** ptr);

/* Marker points and the reference's order travelling WITH the sweep (opt-in; additive under ABI 5).  urf_marker_points and
 * urf_ordered_indices read the scratch row of the sweep waited for last on the context's stream: they wait for every sweep in flight,
 * launch their kernels behind them, synchronise, and answer URF_ERR_BUSY once the row has been resubmitted.  With a bit set here the
 * captured sequence of every sweep submitted afterwards also produces that product on the sweep's own row and stream and copies it to a
 * pinned result buffer of the sweep's slot, as labels and summary are; after urf_classify_pc2_wait it is read per ticket with no further
 * GPU work, for any number of sweeps in flight up to URF_MAX_IN_FLIGHT and any max_batch -- no URF_ERR_BUSY, no second run of a fused
 * row-major sweep, and the context stays fused (independent of urf_set_front_outputs).
 *   urf_set_sweep_outputs   bits: URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER, 0 (default) = off; other bits URF_ERR_INVALID_ARG.
 *                           Allocates everything the sequences need (per scratch row the read-outs' scratch, per slot a device and a
 *                           pinned result buffer of 1448 + 3 * max_points words): URF_ERR_OOM comes from here and leaves the switch as
 *                           it was.  URF_ERR_BUSY while a sweep is in flight.  A change makes every slot capture its sequence again.  A
 *                           context that never turns a bit on allocates and launches nothing.  Labels, summaries, urf_front_scans,
 *                           urf_callback_path_state and batch calls are what they are without it.
 *   urf_result_marker_points    *pts = the ticket's marker points (x, y, z, red per point, as urf_marker_points writes them), *count of them.
 *   urf_result_ordered_indices  *road / *curb / *ring10 = the ticket's lists as urf_ordered_indices writes them (a pointer that is not
 *                           wanted may be NULL), counts[3] their lengths.
 * Both follow urf_result_labels: pointers into the slot's pinned buffer, valid until the slot is used again; a ticket never issued or
 * overtaken URF_ERR_INVALID_ARG, one still in flight URF_ERR_BUSY; a sweep submitted while the product's bit was off
 * URF_ERR_INVALID_ARG (urf_last_error names the switch); a sweep whose status is not URF_OK: count 0, counts {0, 0, 0}.
 * urf_marker_points / urf_ordered_indices / urf_read_stage / urf_front_explain keep working next to them, BUSY rule included. */
#define URF_SWEEP_OUT_MARKER_POINTS 1u
#define URF_SWEEP_OUT_ORDER         2u
int urf_set_sweep_outputs(urf_ctx* ctx, uint32_t bits);
int urf_result_marker_points(urf_ctx* ctx, uint32_t ticket, const float** pts, uint32_t* count);
int urf_result_ordered_indices(urf_ctx* ctx, uint32_t ticket, const uint32_t** road, const uint32_t** curb,
                               const uint32_t** ring10, uint32_t counts[3]);

/* One captured sequence for sweeps of varying length (opt-in; additive under ABI 5).  The sequence a slot replays is keyed by the
 * sweep's number of points: a stream whose sweeps differ in length -- velodyne_pointcloud's default mode, any is_dense cloud, anything a
 * driver-side filter has touched -- captures and instantiates a sequence per sweep.  The reference drops non-finite points before
 * anything else (lidar_segmentation.cpp:100-117) and never looks at an input index, so (NaN, NaN, NaN) points behind a sweep change no
 * label and no summary: with a quantum set, a sweep of n points on the callback path (urf_classify_pc2_async and urf_classify_pc2) runs
 * as n' points, n' the next multiple of the quantum, the last n' - n of them NaN, and every sweep of that n' replays one sequence.
 *   urf_set_sweep_quantum   points: 0 (default) = off, every call launches, copies and captures what it does without the switch; else a
 *                           multiple of 2048 (a tile) and at most the context's max_points, anything else URF_ERR_INVALID_ARG.
 *                           URF_ERR_BUSY while a sweep is in flight; URF_ERR_OOM leaves the switch as it was.  A change forgets every
 *                           captured sequence.  A sweep whose n' exceeds max_points runs unpadded under its own key, as without the
 *                           switch.  Each slot keeps up to URF_SWEEP_SEQS sequences, the least recently used one making room for a
 *                           ninth; whatever invalidates a sequence (parameters, settings, a larger message buffer) drops all of them.
 *                           (8 is a design constant, not a measurement: a sensor's dense sweeps differ by a few tiles, and a larger
 *                           quantum is the caller's lever.)  Off: one sequence per slot.
 * A staged message gets its pad from the host, into the pinned planes; a message a producer wrote into urf_pinned_input's buffer is
 * gathered by a kernel that reads the sweep's own length from a device word of the slot and stores NaN behind it -- the bytes of the
 * pinned buffer behind the n records are never read.  A slot's message buffers grow to the largest message seen, and a new buffer
 * forgets the slot's sequences: with a quantum set they grow to twice the padded length at once (at most max_points), and a producer
 * asks urf_pinned_input for its largest message, not for each one's size.
 * Everything the caller sees is in terms of its own n: urf_classify_pc2_wait copies n label bytes, urf_result_labels promises n bytes,
 * urf_result_ordered_indices and urf_result_marker_points name only indices < n (a NaN point lies on no ring and in no cloud), and
 * urf_read_stage, urf_ordered_indices, urf_marker_points, urf_compact_indices and urf_front_explain after such a sweep accept the byte
 * counts and capacities they accept for the unpadded sweep and answer for its n points.  A sweep the short sequence voided is run again
 * inside urf_classify_pc2_wait as the padded sweep it was.
 *   urf_callback_path_captures   *n_captured = launch sequences captured so far over all slots, for any cause, switch on or off;
 *                           *n_resident = the sequences a sweep submitted now could replay (those of an earlier epoch are released by
 *                           their slot's next submission and not counted).  Either pointer may be NULL. */
#define URF_SWEEP_SEQS 8
int urf_set_sweep_quantum(urf_ctx* ctx, uint32_t points);
int urf_callback_path_captures(const urf_ctx* ctx, uint32_t* n_captured, uint32_t* n_resident);

/* The results of urf_set_sweep_outputs written to host memory at their own size (opt-in; additive under ABI 5).  Without this switch the
 * sequence copies the three lists as three arrays of the sweep's length, 12 bytes per point whatever they hold.  With it the kernels that
 * produce the marker points, their count, the three list counts and the lists store them themselves -- every word once, with plain stores --
 * into a pinned buffer of the sweep's slot that is mapped into the device's address space and coherent (1448 header words +
 * 2 * max_points list words: road and curb are disjoint sets of the sweep's points, ring 10 has at most all of them), and the sequence
 * holds no device-to-host copy for these products (labels and summary are copied as before).  Only the entries that exist cross the link.
 *   urf_set_sweep_results_direct   on: 0 (default) | 1, anything else URF_ERR_INVALID_ARG.  Decides something only together with bits of
 *                           urf_set_sweep_outputs: with none set it allocates and launches nothing; whichever of the two setters comes
 *                           second allocates the buffers (URF_ERR_OOM leaves the switch as it was), and a context that has the switch on
 *                           before the first bit needs no device-side result buffer.  URF_ERR_BUSY while a sweep is in flight.  A change
 *                           makes every slot capture its sequence again.  Off: every call launches and copies what it does without it.
 * urf_result_marker_points and urf_result_ordered_indices keep signature and contract; they return pointers into that buffer.  The lists
 * of a sweep submitted with the switch on lie back to back, independent of the sweep's length (and of its padded length under
 * urf_set_sweep_quantum): *curb == *road + counts[0], *ring10 == *curb + counts[1]; the words behind them are never written.  A slot
 * remembers how its sweep was submitted: the switch may change between the wait and the read.  Everything else -- labels, summaries,
 * urf_marker_points, urf_ordered_indices, urf_read_stage, urf_front_explain, urf_front_scans, batch calls -- is what it is without it. */
int urf_set_sweep_results_direct(urf_ctx* ctx, int on);

/* ---- batch of scans, device-resident ---------------------------------------
 * n_scans independent scans of n_per_scan points each; scan s owns elements
 * [s*n_per_scan, (s+1)*n_per_scan) of d_x/d_y/d_z (SoA, device memory) and of
 * d_labels.  d_info (device, n_scans entries) is optional.  Asynchronous on
 * the context's stream. */
int urf_classify_batch_soa(urf_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                           uint32_t n_per_scan, uint32_t n_scans,
                           uint8_t* d_labels, urf_scan_info* d_info);

/* Same with ragged scans: scan s owns [d_offsets[s], d_offsets[s+1]) (device
 * array of n_scans+1 uint32).  max_len >= the longest scan (host value). */
int urf_classify_batch_soa_ragged(urf_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                  const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                  uint8_t* d_labels, urf_scan_info* d_info);

/* Batch of PointCloud2-layout scans in device memory (n_per_scan records of
 * point_step bytes per scan, scans back to back). */
int urf_classify_batch_pc2(urf_ctx* ctx, const uint8_t* d_data, uint32_t n_per_scan, uint32_t n_scans,
                           uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z,
                           uint8_t* d_labels, urf_scan_info* d_info);

/* The same with ragged scans, as urf_classify_batch_soa_ragged: scan s is records [d_offsets[s], d_offsets[s+1])
 * of d_data (device array of n_scans+1 uint32; every message has the same record layout, back to back), its labels
 * go to the same indices of d_labels.  n_total = d_offsets[n_scans] as a host value (records unpacked; at most
 * max_points * max_batch of the context, else URF_ERR_CAPACITY), max_len >= the longest scan.  A zero-length message
 * gets status URF_TOO_FEW_POINTS (what urf::Detector answers for an empty message).  Labels and summaries equal
 * those of urf_classify_batch_soa_ragged on the same points.  Messages of variable length: drivers that drop
 * non-returns (Velodyne's non-organised mode, any is_dense cloud). */
int urf_classify_batch_pc2_ragged(urf_ctx* ctx, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total, uint32_t max_len, uint32_t n_scans, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint8_t* d_labels, urf_scan_info* d_info);

/* ---- the published clouds of a batch, on the device ---------------------------
 * The four clouds the reference publishes per sweep (lidar_segmentation.cpp:354-367, 605-608, 618-621) for every
 * scan of the LAST classify call, which must have been one of the four batch entry points above (after a sweep of
 * the callback path, or before any call: URF_ERR_INVALID_ARG -- the callback path has urf::Detector).  One record
 * per point, the layout of pcl::PointXYZI and of urf::PointXYZI: x, y, z, intensity copied bit for bit from the
 * input (NaN payloads and -0 survive), w = 1.0f, pad = 0.
 *   d_records   all clouds back to back: scan by scan, inside a scan road, curb, roi, road_probably (the order of
 *               urf_compact_indices' counts); NULL: only counts and offsets are written.  capacity (records) must
 *               be at least 3 * n_scans * max_len of the call (road + curb and road_probably are subsets of roi),
 *               else URF_ERR_CAPACITY.
 *   d_counts    [4 * n_scans]: d_counts[4*s+k] records of cloud k of scan s (0 for a scan whose status is not URF_OK);
 *   d_offsets   [4 * n_scans]: where that cloud starts in d_records (exclusive prefix of d_counts, 64 bit).
 * order: URF_ORDER_INPUT, all four clouds in input order (urf::Detector's default), or URF_ORDER_REFERENCE: road,
 * curb and road_probably in exactly the sequence urf_ordered_indices_batch returns, roi in input order.  The
 * reference order runs urf_ordered_indices_batch's kernels and so inherits what it does after a call that took the
 * fused front end (the call runs once more through the general kernels, and the context stays with them); input
 * order reads nothing but the labels and the inputs.  Layout and values do not depend on scheduling.  Asynchronous
 * on the context's stream, results stay on the device.
 * urf_clouds_batch_soa: the last call was urf_classify_batch_soa(_ragged); x / y / z are read from that call's
 * arrays, intensity from d_intensity (device, laid out like x; NULL: intensity 0).
 * urf_clouds_batch_pc2: the last call was urf_classify_batch_pc2(_ragged); the caller passes the same message
 * bytes again, x / y / z / intensity are read from the records (off_intensity = -1: the messages have no FLOAT32
 * intensity field, intensity 0 -- what pcl::fromROSMsg leaves; otherwise off_intensity + 4 <= point_step).
 * LIFETIME (as for urf_ordered_indices* below): the last call's d_labels must still be alive and unmodified, and so
 * must its inputs -- d_x / d_y / d_z of a SoA call, d_data of a PointCloud2 call -- until these calls have completed. */
typedef struct urf_point_xyzi {
    float x, y, z, w;       /* w = 1.0f */
    float intensity;
    float pad[3];           /* 0 */
} urf_point_xyzi;           /* 32 bytes */
#define URF_ORDER_INPUT     0
#define URF_ORDER_REFERENCE 1
int urf_clouds_batch_soa(urf_ctx* ctx, const float* d_intensity, int order, urf_point_xyzi* d_records, uint64_t capacity, uint32_t* d_counts, uint64_t* d_offsets);
int urf_clouds_batch_pc2(urf_ctx* ctx, const uint8_t* d_data, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, int32_t off_intensity, int order, urf_point_xyzi* d_records, uint64_t capacity, uint32_t* d_counts, uint64_t* d_offsets);

/* ---- index-set outputs -----------------------------------------------------
 * Compacts the label bytes of ONE scan (device) into ascending index lists
 * (device, each with room for n_points entries; any may be NULL) and writes
 * the four counts to d_counts[0..3] = {road, curb, roi, road_probably}. */
int urf_compact_indices(urf_ctx* ctx, const uint8_t* d_labels, uint32_t n_points,
                        uint32_t* d_road, uint32_t* d_curb, uint32_t* d_roi, uint32_t* d_ring10,
                        uint32_t* d_counts);
/* The same for every scan of a batch in one launch (grid over tiles x scans, asynchronous on the
 * context's stream): scan s owns [s*n_per_scan, (s+1)*n_per_scan) of d_labels and of every list
 * (indices are relative to the scan), and d_counts[4*s .. 4*s+3].  The reference builds these sets
 * for every sweep (lidar_segmentation.cpp:354-367, 605-608). */
int urf_compact_indices_batch(urf_ctx* ctx, const uint8_t* d_labels, uint32_t n_per_scan, uint32_t n_scans,
                              uint32_t* d_road, uint32_t* d_curb, uint32_t* d_roi, uint32_t* d_ring10,
                              uint32_t* d_counts);

/* ---- the published clouds, in the reference's order ------------------------
 * The reference fills "road", "curb" and "road_probably" ring by ring (sorted
 * ring index ascending), each ring in ascending azimuth (its per-ring quicksort,
 * lidar_segmentation.cpp:70-93, 289-291, 354-367, 605-608); "roi" is in input
 * order.  After a classify call this returns the input indices of scan `scan`
 * in exactly that order (points of one ring with bit-identical azimuths in the
 * order the reference's quicksort leaves them in: it is run literally for such a
 * ring).  Host buffers with room
 * for n_points entries each (any may be NULL); counts[3] = {road, curb,
 * road_probably}.  Synchronous; costs one extra per-ring sort.
 * COST of bit-identical azimuths: a ring that holds ONE such pair is sorted a second time by the reference's own quicksort, run
 * literally by a single wave -- the ring is nearly sorted by then, Lomuto's scheme is quadratic on that: about 1 ms per ring of
 * 2048 points (the same holds for urf_marker_points and for a ring with a NaN azimuth).  A sensor that delivers exact duplicates
 * (dual returns written twice) in many rings makes these two entry points tens of milliseconds slower; the labels are not affected.
 * LIFETIME: urf_ordered_indices*, urf_marker_points* and urf_read_stage run kernels over the LAST classify call's results, which
 * include buffers of the caller's.  d_labels of that call is always among them and must stay allocated and unmodified until the last of
 * these calls on it has completed (for a sweep of the callback path the library owns that buffer: nothing to keep alive).  After a call
 * through the general kernels nothing else is: the x / y / z these kernels need were copied into the context's scratch by the call
 * itself.  A call that took the fused front end (below) kept no such copies, so its INPUT must stay alive as well -- x / y / z of a
 * SoA call; a PointCloud2 call's staged copy is the context's -- in either position of urf_set_front_outputs: with the switch off the
 * call is run again from it (and d_labels rewritten with the same bytes), with the switch on x / y / z and d_labels are read where
 * they are and nothing of the caller's is written.  urf_clouds_batch_* (above) read the last batch call's inputs in any case:
 * x / y / z of a SoA call, the message bytes of a PointCloud2 call. */
int urf_ordered_indices(urf_ctx* ctx, uint32_t scan, uint32_t* road, uint32_t* curb, uint32_t* ring10,
                        uint32_t* counts);
/* Every scan of the last classify call at once, results on the DEVICE (asynchronous on the
 * context's stream): list l of scan s at d_l + s*stride (stride >= the call's scan length; any list
 * may be NULL), d_counts[3*s .. 3*s+2] = {road, curb, road_probably}. */
int urf_ordered_indices_batch(urf_ctx* ctx, uint32_t* d_road, uint32_t* d_curb, uint32_t* d_ring10,
                              uint32_t stride, uint32_t* d_counts);

/* ---- road_marker: the marker points ------------------------------------------
 * lidar_segmentation.cpp:295-351: for every integer degree i = 0..360 the farthest road point
 * with azimuth in [i, i+1), scanning ring by ring (each ring in ascending azimuth) until the first
 * point of that degree that is not road; `red` tells whether such a point was met.  After a
 * classify call this returns the marker points of scan `scan`: pts[4*k + 0..3] = x, y, z, red
 * (host buffer with room for 361 points), *count = their number (the reference's cM).
 * The line strips the reference builds from them (colour grouping, Douglas-Peucker
 * simplification, ghost deletion, :369-602): urf_marker_strips* below, urf::Detector::road_marker().
 * Synchronous; costs one extra per-ring sort. */
int urf_marker_points(urf_ctx* ctx, uint32_t scan, float* pts, uint32_t* count);
/* Every scan of the last classify call at once, results on the DEVICE (asynchronous): the marker
 * points of scan s at d_pts + s*361*4 (x, y, z, red per point), their number in d_counts[s]. */
int urf_marker_points_batch(urf_ctx* ctx, float* d_pts, uint32_t* d_counts);

/* The polygon parameters of the reference (cfg/LidarFilters.cfg:75-84 -> main.cpp:29-32). */
typedef struct urf_marker_params {
    uint32_t size;              /* = sizeof(urf_marker_params) */
    int32_t  simple_poly_allow; /* cfg:75  bool, default true */
    float    poly_s_param;      /* cfg:78  Douglas-Peucker distance, default 0.7 */
    float    poly_z_manual;     /* cfg:81  default -1.5 */
    int32_t  poly_z_avg_allow;  /* cfg:84  bool, default true */
} urf_marker_params;
int urf_default_marker_params(urf_marker_params* p);

/* The line simplification of the polygon step (lidar_segmentation.cpp:475,512,548 call
 * boost::geometry::simplify(line, out, poly_s_param)): Douglas-Peucker with the distance of a point
 * to the SEGMENT between the span's ends, first and last point kept, an interior point kept iff it
 * is the farthest of its span and strictly farther than max_distance; float coordinates
 * (point_xy<float>, data_structures.hpp:38).  xy = n points (x0, y0, x1, y1, ...); keep[i] = 1 for
 * the points of the simplified line.  Boost.Geometry itself is not in the reference checkout:
 * the behaviour is pinned by the worked example of its documentation (tests/test_simplify_kat.py). */
int urf_simplify_line(const float* xy, uint32_t n, float max_distance, uint8_t* keep);

/* ---- road_marker: the line strips ------------------------------------------------
 * lidar_segmentation.cpp:369-602: what the reference publishes as "road_marker" for a sweep with more than two marker
 * points -- the colour fix-ups (:381-415), one LINE_STRIP marker per run of equal colour (green = free, red = a non-road
 * point ended the degree's beam; the segment that joins two runs is red, so joint points appear twice), each optionally
 * replaced by its Douglas-Peucker outline at height poly_z_manual (simple_poly_allow), every z optionally replaced by the
 * sweep's running-mean height (poly_z_avg_allow), and DELETE markers for the strips of the previous publishing sweep that this
 * one no longer has (:591-598).  One record per marker and a packed point array; all values float: every coordinate the
 * reference stores in its double geometry_msgs::Point is a float widened.
 * STATE between sweeps: the ghost count = the id of the last ADD marker of the latest sweep that published (the reference's
 * `ghostcount`), nothing else (DESIGN.md section 4 derives why the reference's member linestring never carries points over).
 * A sweep with count <= 2 publishes nothing and leaves it alone.  A ghost count is at most URF_MARKER_MAX_STRIPS - 1 (the id
 * of the last of URF_MARKER_MAX_STRIPS strips); incoming values outside [0, URF_MARKER_MAX_STRIPS - 1] are clamped to that
 * range -- the largest value a sweep can leave, and the largest for which ADD + DELETE markers fit URF_MARKER_MAX_STRIPS records.
 * BOUNDS: after the fix-ups every run of equal colour holds at least two of the at most 361 marker points, so a sweep has at
 * most 180 strips and 361 + 179 points (each of the 179 joints once more), both reached by 361 points in runs of 2, 2, ..., 3;
 * DELETE markers only fill up to the previous sweep's strip count. */
typedef struct urf_marker_strip {
    int32_t  id;                    /* Marker::id; DELETE markers carry the reference's ids (last ADD id + 1 ...) */
    int32_t  action;                /* URF_MARKER_ADD or URF_MARKER_DELETE */
    float    r, g, b, a;            /* a DELETE marker keeps the last strip's colour, as in the reference */
    uint32_t first_point, n_points; /* into the sweep's xyz; a DELETE marker has 0 points */
} urf_marker_strip;                 /* 32 bytes */
#define URF_MARKER_ADD              0
#define URF_MARKER_DELETE           2
#define URF_MARKER_MAX_POINTS       361   /* marker points per sweep (urf_marker_points) */
#define URF_MARKER_MAX_STRIPS       180   /* markers (ADD + DELETE) per sweep */
#define URF_MARKER_MAX_STRIP_POINTS 540   /* strip points per sweep */
/* One sweep on the host (no context, no device): pts = count x {x, y, z, red} as urf_marker_points returns them (count at
 * most 361, red exactly 0 or 1, else URF_ERR_INVALID_ARG), *ghostcount in / out (see STATE).  *published = 0 / 1 (0: no
 * MarkerArray for this sweep, n_strips = n_points = 0, *ghostcount untouched), strips with room for URF_MARKER_MAX_STRIPS
 * records, xyz for 3 * URF_MARKER_MAX_STRIP_POINTS floats.  urf::MarkerBuilder runs the same code. */
int urf_marker_strips(const float* pts, uint32_t count, const urf_marker_params* mp, int32_t* ghostcount, int32_t* published,
                      urf_marker_strip* strips, uint32_t* n_strips, float* xyz, uint32_t* n_points);
/* A batch on the device, asynchronous on the context's stream.  A pure function of its arguments (the context lends its
 * stream and one word of scratch): d_pts / d_counts are laid out as urf_marker_points_batch writes them (scan s: 361 * 4
 * floats at d_pts + s * 361 * 4, its count in d_counts[s]; counts above 361 are read as 361), so the two calls chain without
 * the host.  Scan s writes its markers at d_strips + s * URF_MARKER_MAX_STRIPS, its points at
 * d_xyz + 3 * s * URF_MARKER_MAX_STRIP_POINTS, and d_n[3*s .. 3*s+2] = published (0 / 1), markers, points (0, 0, 0 for a scan
 * with count <= 2); bytes of the fixed-stride outputs beyond a scan's counts are unspecified.  Records equal
 * urf_marker_strips' bit for bit.
 * sequence = 1: the scans are consecutive sweeps of one sensor.  Scan 0 starts from *d_ghost (device int32_t; NULL: 0 and
 * nothing is written back), every scan from the nearest earlier scan of the call that publishes, and the value the last
 * publishing scan leaves (the incoming one, unclamped, if none publishes: urf_marker_strips leaves it alone too) is written to *d_ghost, so consecutive calls chain on the
 * device.  sequence = 0: independent scans, each starts from 0 (no DELETE markers); d_ghost is ignored.
 * n_scans above the context's max_batch: URF_ERR_CAPACITY; n_scans = 0 is a no-op.  A red value other than 0 is read as 1. */
int urf_marker_strips_batch(urf_ctx* ctx, const urf_marker_params* mp, const float* d_pts, const uint32_t* d_counts,
                            uint32_t n_scans, int sequence, int32_t* d_ghost, urf_marker_strip* d_strips, float* d_xyz,
                            uint32_t* d_n);

/* ---- stage-wise inspection (parity tests) ----------------------------------
 * After a classify call, copies one intermediate array of scan `scan` to host
 * memory.  Arrays indexed by input point have n_points entries; values of
 * points outside the ROI / not on a ring are unspecified unless noted. */
typedef enum urf_stage {
    URF_STAGE_VALPHA = 1,     /* float  per point: vertical angle, lidar_segmentation.cpp:151-166;
                                 negative for points outside the ROI */
    URF_STAGE_RING = 2,       /* int16  per point: sorted ring index or -1, lidar_segmentation.cpp:226-233 */
    URF_STAGE_AZIMUTH = 3,    /* float  per point: azimuth alpha [deg], lidar_segmentation.cpp:248-269 */
    URF_STAGE_RANGE2D = 4,    /* float  per point: planar d, lidar_segmentation.cpp:245 */
    URF_STAGE_DETECT = 5,     /* uint8  per point on a ring: bit0 star, bit1 x_zero, bit2 z_zero hit (0 elsewhere) */
    URF_STAGE_SECTOR = 6,     /* int16  per point: star sector or -1, star_shaped_search.cpp:171 */
    URF_STAGE_ANGLE_TABLE = 7,/* float[channels]: sorted ring-angle table, lidar_segmentation.cpp:205 */
    URF_STAGE_MAXDIST = 8,    /* float[channels]: maxDistance, lidar_segmentation.cpp:271-274 */
    URF_STAGE_QUADRANTS = 9,  /* float[4]: q1..q4, blind_spots.cpp:13-57 */
    URF_STAGE_BEAM_STOP = 10  /* int16[2*361]: first blocked ring per forward / backward beam
                                 (n_rings = not blocked, -1 = beam not cast) */
} urf_stage;
int urf_read_stage(urf_ctx* ctx, urf_stage what, uint32_t scan, void* host_dst, size_t bytes);
/* Capture mode (default 0 = off: the production path records nothing per input point):
 *   1  every point takes the reference's exact arithmetic and the values are stored: all stages
 *      can be read (URF_STAGE_VALPHA, URF_STAGE_AZIMUTH and URF_STAGE_RANGE2D only in this mode --
 *      without it the pipeline settles most ring / sector / road decisions on float approximations
 *      of these angles and never evaluates the reference's exact value for such a point);
 *   2  the production decisions, with the ring and sector of every input point recorded
 *      (URF_STAGE_RING, URF_STAGE_SECTOR; mode 0 keeps them only in sorted order).
 * The other stages can be read in every mode.  urf_read_stage, urf_ordered_indices and
 * urf_marker_points look at the LAST classify call of the context with the parameters that call
 * ran with; the label buffer handed to that call must still be alive (see LIFETIME above). */
int urf_enable_stage_capture(urf_ctx* ctx, int mode);

/* ---- the fused front end for batches of sweeps in firing order (round 6) -------
 * A batch call (urf_classify_batch_*) whose scans arrive as a spinning LiDAR's driver delivers them -- firing after
 * firing, the `channels` (64, 32 or 16) lasers of a firing in one fixed order (any order): point f * channels + l is laser slot l of
 * firing f, returns missing where there were none -- is classified
 * by a front end that keeps no ring-sorted copy of the sweep (urban_road_filter_amd/csrc/urf_front.hpp: one lane per
 * laser, the detectors' windows of lidar_segmentation.cpp:280-283 / x_zero_method.cpp:30-67 / z_zero_method.cpp:21-72
 * in registers).  Decided per scan on the device; a scan without that shape takes the general kernels in the same
 * call; labels and summaries are identical either way.  Applies with channels == 64, 32 or 16 (the caller states the sensor's
 * laser count through `channels`, as the reference's user does in lidar_segmentation.cpp:4; a 32-laser sweep classified with channels
 * == 64 is handed back to the general kernels), curbPoints == 5, no stage capture, at most 128 x 2048 points per scan (128 tiles of 2048
 * points; 256 tiles with urf_set_front_long_sweeps, below).  Row-major
 * organised clouds (below) have `channels` rows: point l * W + f.  mode 0: never; 1 (default): batch calls of at least 192 scans with channels == 64; with channels == 16 or 32 mode 1 never takes the fused
 * kernels -- no batch size, no row-major sighting, not on the callback path: they are opt-in through mode 2 until their crossover has been
 * measured (tools/front_lasers_bench.py) -- (below that the general kernels are faster: a sweep's fused kernels are
 * a few long dependent chains, which need many sweeps side by side to fill the device; a context whose sweeps have turned out to be
 * row-major takes the fused kernels at any batch size -- the general kernels are 2.3 x slower on that layout even for four sweeps --
 * and on the callback path: urf_classify_pc2(_async) of a row-major sweep, from the context's second or third such sweep on); 2: every
 * batch call it applies to; 3: as 2 in everything (batch sizes, row-major sweeps, 16 / 32 lasers), and with channels == 64 additionally
 * curbPoints 1..8 instead of 5 only: one instance of the march and of its finish per value, the detectors' window of 2 * curbPoints + 1
 * heights in registers; chosen per call from the parameters in force (with curbPoints == 5 mode 3 launches the very kernels of modes 1
 * and 2).  curbPoints 9..30 keep the general kernels in every mode; channels 16 / 32 with curbPoints != 5 keep them in every mode unless
 * urf_set_front_curb_points (below) is on, which extends mode 3 to them; modes 1 and 2 keep them
 * for every curbPoints != 5.  urf_set_params starts the captured per-slot sequences of the callback path afresh, so a row-major
 * context in mode 3 whose curbPoints changes stays on the fused kernels there, with the instance for the new value.  Mode 3 is opt-in:
 * its times are in profiles/curb_points_bench.json.  urf_read_stage / urf_ordered_indices* / urf_marker_points* read ring-sorted intermediate
 * results: after a call that took the fused front end they first run that call again through the general kernels
 * (the call's INPUT arrays must then still be alive, like its label buffer), and the context stays with the general
 * kernels afterwards (until urf_set_front_mode is called again with a mode other than 0).  urf_set_front_outputs(ctx, 1) spares
 * urf_ordered_indices*, urf_clouds_batch_* (reference order) and urf_marker_points* that second run and its consequence.  A context that has handed a
 * scan back launches the general kernels as full grids next to the fused ones from then on, and one that has handed a
 * whole batch back (unorganised clouds) stops trying in mode 1; urf_set_params with other parameters and
 * urf_set_front_mode with another mode forget both.  urf_front_scans: how many scans of the last batch call took the
 * fused front end (synchronises); a scan that kept its flag but has no result -- fewer than 30 points in the region of interest: nothing
 * is published for it by either kind of kernel -- is counted.
 * One rule of capacity next to the rules of shape: the points whose detector decision is still open after the march wait in a list of
 * max_points / 8 entries per scan (at least 4096; max_points as given to urf_create), which sweeps of a thousand firings and more
 * never fill.  A sweep of a few hundred firings, whose neighbours on a ring lie more than a degree apart, leaves a quarter of its points
 * and more there: in a context created for just its size the list overflows and the scan is handed back (same labels); a context
 * created for sixteen times the points has room for every one.
 *
 * 128 lasers per firing (urf_set_front_lasers128, k_front128* in urban_road_filter_amd/csrc/urf_front.hpp): with the switch on, channels == 128 and
 * curbPoints == 5, modes 2 and 3 -- never modes 0 and 1 -- also take sweeps of 128 lasers per firing, in firing order (point f * 128 + l)
 * or row-major (128 rows; sighted by one call, fused from the next on, the callback path included): one wave per block of the march, two
 * lasers (l and l + 64) per lane.  Everything above holds for them as well -- per-scan hand-back, identical labels and summaries,
 * urf_front_scans -- and so does the limit of 128 x 2048 points per scan: a 128 x 4096 sweep keeps the general kernels unless
 * urf_set_front_long_sweeps is on as well.  Every
 * 128-laser table entry is a ring to these kernels, entry 127 included (their records keep the ring in eight bits).  curbPoints != 5
 * keeps the general kernels at 128 lasers unless urf_set_front_curb_points (below) is on as well, in mode 3.  The switch is off by default and opt-in whatever tools/front_lasers_bench.py --lasers128
 * measures; turning it on allocates the per-scan tables these kernels need (URF_ERR_OOM: it stays off).
 *
 * Long sweeps (urf_set_front_long_sweeps): the limit of 128 tiles is the finish step's, which keeps a presence word and a count per
 * (tile, laser slot) in LDS.  With the switch on, modes 2 and 3 -- never modes 0 and 1 -- also take batch calls whose longest scan has
 * 129..256 tiles of 2048 points (256 tiles: a 128 x 4096 sweep; a 128-laser unit at 0.1 degree steps delivers 225, a 64-laser unit at
 * 0.08 degrees 141), at every laser count the front end knows (16, 32, 64; 128 behind urf_set_front_lasers128), in firing order and
 * row-major, ragged batches, the callback path's row-major sweeps and the read-outs of urf_set_front_outputs included: the same
 * kernels, the finish step with the LDS that many tiles need (108 KiB at 256 tiles: one workgroup per CU).  A call of at most 128 tiles
 * launches exactly what it launches with the switch off; a call of more than 256 tiles keeps the general kernels.  Opt-in: its times
 * are in profiles/front_long_bench.json.
 *
 * curbPoints 1..8 at 16, 32 and 128 lasers (urf_set_front_curb_points): mode 3's instances for curbPoints other than 5 exist at 64 lasers
 * only unless this switch is on.  With it, mode 3 -- never modes 0, 1 and 2 -- also takes curbPoints 1..8 with channels == 16 or 32
 * (k_front32_cp*, k_front16_cp*: the march of mode 3 with half or a quarter of the wave's lanes; the finish step is the 64-laser one, which
 * takes the laser count at run time), and with channels == 128 when urf_set_front_lasers128 is on as well (k_front128_cp*,
 * k_front_finish128_cp*, urban_road_filter_amd/csrc/urf_front.hpp: two windows of 2 * curbPoints + 1 heights per lane).  Everything
 * above keeps its meaning with these instances: per-scan hand-back, identical labels and summaries, urf_front_scans, ragged batches,
 * row-major sightings and the callback path's row-major sweeps, urf_set_front_long_sweeps, urf_set_front_outputs, the dense entry
 * points.  curbPoints 9..30 keep the general kernels everywhere; with the switch off every call launches exactly what it launched
 * before the switch existed.  Opt-in: its times are in profiles/curb_points_lasers_bench.json.
 *
 * Firings that span several star sectors (urf_set_front_multi_sector): the fused kernels want the points of a firing that take part in the
 * star-shaped search to share one sector, and the sectors not to fall inside a tile of 2048 points.  No real spinning LiDAR delivers that:
 * the unit turns while a firing is shot (VLP-16, HDL-32E), its lasers carry fixed azimuth offsets (VLP-32C, HDL-64E, a staggered Ouster
 * cloud), and a sweep that does not start on a tile border has its seam (sector K - 1 -> 0) inside a tile.  With the switch off such a
 * scan is handed back to the general kernels.  With it on, the star-shaped search on and curbPoints == 5, every front mode that takes a
 * call launches the k_front*_ms instance of the march (16, 32, 64 lasers; 128 behind urf_set_front_lasers128), which accepts any sector
 * per participant, and k_front_sectors behind it (urban_road_filter_amd/csrc/urf_k_front_sectors.hpp), which puts every tile's star records in
 * sector order; everything downstream is unchanged, labels and summaries are identical.  Every OTHER rule of the shape still hands a scan
 * back (one laser, one ring; ranges; a ring point on the sensor's axis; unorganised clouds).  curbPoints 1..4 and 6..8 (mode 3) keep
 * their plain instances and with them the hand-back of such scans unless urf_set_front_multi_sector_curb_points (below) is on as well;
 * with the star-shaped search off sectors do not matter and the plain
 * kernel is launched.  Firing order, row-major, ragged batches, the callback path's row-major sweeps, urf_set_front_long_sweeps,
 * urf_set_front_outputs and the dense entry points keep their meaning.  With the switch off every call launches exactly what it launched
 * before the switch existed.  Turning it on allocates two bytes per scratch element (URF_ERR_OOM: it stays off).  Opt-in: its times are in
 * profiles/front_multi_sector_bench.json.
 *
 * ... at curbPoints 1..8 (urf_set_front_multi_sector_curb_points): the multi-sector march exists for curbPoints 5 only unless this switch
 * is on.  With it on AND urf_set_front_multi_sector on, a call that takes the fused kernels with the star-shaped search on and curbPoints
 * 1..4 or 6..8 launches the k_front*_ms_cp<n> instance of the march (the window of 2 * curbPoints + 1 heights of k_front*_cp<n>, any
 * sector per participant) with k_front_sectors behind it; the finish step is the plain one of that curbPoints.  Whether such a call takes
 * the fused kernels at all is decided as before: front mode 3 at 64 lasers, urf_set_front_curb_points on top of it at 16, 32 and 128,
 * urf_set_front_lasers128 for 128.  The switch decides nothing with urf_set_front_multi_sector off, in front modes below 3, with the
 * star-shaped search off, at curbPoints 5 and at curbPoints 9..30, and it allocates nothing.  Labels and summaries are identical; with the
 * switch off every call launches exactly what it launched before the switch existed.  Opt-in: its times (64 lasers, curbPoints 3
 * and 8) are in profiles/front_multi_sector_cp_bench.json. */
int urf_set_front_mode(urf_ctx* ctx, int mode);
int urf_front_scans(urf_ctx* ctx, uint32_t* n_fused);
/* 0 (default): as today.  1: with channels == 128 and curbPoints == 5, front modes 2 and 3 also send sweeps of 128 lasers per
 * firing (firing order: point f * 128 + l; row-major: 128 rows) through the fused front end.  Forgets sightings / hand-backs
 * like urf_set_front_mode.  Anything else: URF_ERR_INVALID_ARG. */
int urf_set_front_lasers128(urf_ctx* ctx, int on);
/* 0 (default): as today, the fused front end takes scans of at most 128 tiles (128 x 2048 points).  1: front modes 2 and 3 also send
 * batch calls whose longest scan has 129..256 tiles through it (longer ones keep the general kernels).  Forgets sightings / hand-backs
 * like urf_set_front_mode.  A device that does not grant a workgroup the LDS the finish step needs at 256 tiles: URF_ERR_OOM, and the
 * switch stays off.  Anything else: URF_ERR_INVALID_ARG. */
int urf_set_front_long_sweeps(urf_ctx* ctx, int on);
/* 0 (default): as today, front mode 3 takes curbPoints other than 5 with channels == 64 only.  1: front mode 3 also takes curbPoints
 * 1..8 with channels == 16 or 32, and with channels == 128 when urf_set_front_lasers128 is on; modes 0, 1 and 2 never do.  Forgets
 * sightings / hand-backs like urf_set_front_mode.  Anything else: URF_ERR_INVALID_ARG. */
int urf_set_front_curb_points(urf_ctx* ctx, int on);
/* 0 (default): as today, a scan whose firings span several star sectors, or whose sectors fall inside a tile, is handed back to the
 * general kernels.  1: with the star-shaped search on and curbPoints == 5 the fused front end keeps such a scan (k_front*_ms and
 * k_front_sectors, above); other curbPoints keep the plain instances.  Forgets sightings / hand-backs like urf_set_front_mode.
 * URF_ERR_OOM: the switch stays off.  Anything else: URF_ERR_INVALID_ARG. */
int urf_set_front_multi_sector(urf_ctx* ctx, int on);
/* 0 (default): as today, urf_set_front_multi_sector applies to curbPoints == 5 only.  1: it applies to every curbPoints the call's fused
 * kernels have an instance for (1..8: front mode 3, urf_set_front_curb_points), through k_front*_ms_cp<n>; nothing changes while
 * urf_set_front_multi_sector is off.  Allocates nothing.  Forgets sightings / hand-backs like urf_set_front_mode.  Anything else:
 * URF_ERR_INVALID_ARG. */
int urf_set_front_multi_sector_curb_points(urf_ctx* ctx, int on);
/* 0 (default): after a call that took the fused front end, urf_ordered_indices*, urf_clouds_batch_* with
 * URF_ORDER_REFERENCE and urf_marker_points* first run that call again through the general kernels, and the context stays with those.
 * 1: these read-outs take a fused call's results as they are (urban_road_filter_amd/csrc/urf_k_front_outputs.hpp: the rings' points
 * in order from the front end's presence words, per scan on the device; a scan that was handed back is read as ever): no second
 * run, urf_front_scans still reports the call, the next batch call is fused again without a urf_set_front_mode, the caller's d_labels
 * and x / y / z (SoA; PointCloud2: the context's staged copy) are read and never written -- they must stay alive and unmodified until
 * the read-out has completed.  Same lists and marker points, bit for bit; 16, 32, 64 and 128 lasers, every fused curbPoints, firing
 * order and row-major, the callback path's fused sweeps included.  urf_read_stage keeps the second run in either position: stage
 * values are defined as the general kernels'.  The switch decides nothing about which kernels classify and forgets no sighting or
 * hand-back.  The read-outs' scratch grows with their first use (URF_ERR_OOM from that call).  Anything else: URF_ERR_INVALID_ARG. */
int urf_set_front_outputs(urf_ctx* ctx, int on);

/* ---- urf_front_explain: why a scan of the last call left the fused front end, and what keeps it -----------------
 * Labels are the same on either path, so nothing else tells a caller that a stream of sweeps runs on the slower kernels.  The function
 * reads "the last call" like the other read-outs -- a batch call: n = its scans; a sweep of the callback path that has been waited for:
 * n = 1, URF_ERR_BUSY once its scratch row has been resubmitted; a dense call: the PADDED batch, firing order -- and writes one record per
 * scan to `out` (host memory).  layout: how the caller's sweeps are organised, 0 firing order (point f * channels + l), 1 row-major (point
 * l * F + f).  It synchronises.  LIFETIME: the call's input arrays must still be alive and unmodified, as for urf_ordered_indices*.
 * No call yet, n other than the call's scans, a layout other than 0 / 1, a null pointer: URF_ERR_INVALID_ARG -- except out == NULL with
 * n == 0, which asks how many records the last call has: the function returns that number (0: no call yet) and does nothing else.
 *
 * It changes nothing in the context: no second run, no hand-back or sighting forgotten, the context does not turn to the general kernels
 * (unlike the read-outs above), the next classify call launches exactly what it would have launched.  Its scratch grows with its first use
 * (URF_ERR_OOM from that call); a context that never calls it allocates and launches nothing for it.
 *
 *   fused   1: the scan's flag is still set -- what urf_front_scans counts.
 *   call    URF_WHY_CALL_*: the terms of the CALL's decision (the same for every scan) that were false; 0 exactly when the call
 *           launched the fused kernels.
 *   scan    URF_WHY_SCAN_*: the rules of the march this scan breaks under the call's settings, whether or not the call launched the fused
 *           kernels.  k_front_explain (urf_k_front_explain.hpp) decides per point what the march decides -- region of interest, ring by the
 *           reference's exact sequence against the scan's final ring table, star sector and participation (beam filter included) -- and
 *           counts; the counters are always reported (star-shaped search off: the three sector counters are 0).  MULTI_SECTOR and
 *           SECTORS_FALL are set only when the call ran, or would have run, without urf_set_front_multi_sector's march; CANDIDATES is
 *           observed (the scan filed more entries than the list holds) and only set when the call ran the march.  A scan with
 *           URF_TOO_FEW_POINTS, or an empty one: scan = 0 and the counters 0.
 *           OTHER: the scan was handed back, the call's decision and every rule above are clean.  Then a speculation of the call was
 *           repaired -- the ring table's look-ahead, the ring-count hint, the rows' table: the repair leaves no word behind, and the next
 *           call does without that speculation -- or the scan broke a rule this function does not know.
 *   advice  URF_ADVICE_*: the smallest change of settings that makes every false term of `call` true, plus what the scan's bits ask for
 *           (MULTI_SECTOR / SECTORS_FALL: urf_set_front_multi_sector, and urf_set_front_multi_sector_curb_points when curbPoints != 5;
 *           CANDIDATES: CAPACITY; ROWS_SIGHTING, OTHER: CALL_AGAIN; the four shape bits and ROWS_LENGTH: NEVER).  With NEVER no setting
 *           helps -- channels not 16 / 32 / 64 / 128, curbPoints 9..30, more than 256 tiles per scan, a sweep that is not organised as
 *           `layout` says (look at params.channels and params.interval) --; the other bits still name what else was missing.
 *   The function cannot tell hand-backs apart that leave nothing behind (OTHER), and it does not see the sticky general context as a
 *   property of the scan: READOUT in `call` says that a read-out turned the context to the general kernels (RESET: urf_set_front_mode
 *   again; FRONT_OUTPUTS: urf_set_front_outputs keeps it from happening again). */
#define URF_WHY_CALL_MODE_OFF     0x001u   /* urf_set_front_mode(ctx, 0) */
#define URF_WHY_CALL_STOPPED      0x002u   /* mode 1 stopped trying after a whole batch was handed back */
#define URF_WHY_CALL_READOUT      0x004u   /* a read-out of ring-sorted results: the context stays with the general kernels */
#define URF_WHY_CALL_CAPTURE      0x008u   /* stage capture is on */
#define URF_WHY_CALL_LASERS       0x010u   /* params.channels has no fused kernels under the settings */
#define URF_WHY_CALL_CURB_POINTS  0x020u   /* params.curbPoints has no fused instance under the settings */
#define URF_WHY_CALL_TILES        0x040u   /* the call's longest scan has more tiles of 2048 points than the settings take */
#define URF_WHY_CALL_FEW_SCANS    0x080u   /* a batch call below mode 1's threshold */
#define URF_WHY_CALL_CALLBACK     0x100u   /* a sweep of the callback path in firing order */
#define URF_WHY_SCAN_LANE_TWO_RINGS 0x001u
#define URF_WHY_SCAN_RING_TWO_LANES 0x002u
#define URF_WHY_SCAN_AXIS           0x004u
#define URF_WHY_SCAN_RANGE          0x008u
#define URF_WHY_SCAN_ROWS_LENGTH    0x010u   /* layout 1 and the scan's length is not `channels` whole rows */
#define URF_WHY_SCAN_MULTI_SECTOR   0x020u
#define URF_WHY_SCAN_SECTORS_FALL   0x040u
#define URF_WHY_SCAN_CANDIDATES     0x080u
#define URF_WHY_SCAN_ROWS_SIGHTING  0x100u   /* layout 1 and the call's sequence had no probe / transpose: the first call only sights */
#define URF_WHY_SCAN_OTHER          0x200u
#define URF_ADVICE_MODE_2          0x0001u   /* urf_set_front_mode(ctx, 2) */
#define URF_ADVICE_MODE_3          0x0002u   /* urf_set_front_mode(ctx, 3) */
#define URF_ADVICE_LASERS128       0x0004u   /* urf_set_front_lasers128 */
#define URF_ADVICE_LONG_SWEEPS     0x0008u   /* urf_set_front_long_sweeps */
#define URF_ADVICE_CURB_POINTS     0x0010u   /* urf_set_front_curb_points */
#define URF_ADVICE_MULTI_SECTOR    0x0020u   /* urf_set_front_multi_sector */
#define URF_ADVICE_MULTI_SECTOR_CP 0x0040u   /* urf_set_front_multi_sector_curb_points */
#define URF_ADVICE_FRONT_OUTPUTS   0x0080u   /* urf_set_front_outputs: read-outs without the second run */
#define URF_ADVICE_RESET           0x0100u   /* call urf_set_front_mode again: it forgets hand-backs and the sticky read-out */
#define URF_ADVICE_CAPTURE_OFF     0x0200u   /* urf_enable_stage_capture(ctx, 0) */
#define URF_ADVICE_BATCH           0x0400u   /* the callback path in firing order: use a batch call */
#define URF_ADVICE_NEVER           0x0800u   /* no setting helps */
#define URF_ADVICE_CAPACITY        0x1000u   /* a context created for more points per scan has a longer candidate list */
#define URF_ADVICE_CALL_AGAIN      0x2000u   /* the next call of the same kind does without what this one tried first */
typedef struct urf_front_why {
    uint32_t fused;                  /* 1: the scan's flag is still set (what urf_front_scans counts) */
    uint32_t call, scan, advice;     /* URF_WHY_CALL_*, URF_WHY_SCAN_*, URF_ADVICE_* */
    uint32_t lanes_two_rings, rings_two_lanes, axis_points, range_points;   /* laser slots that meet two rings; rings fed by two slots; ring points
                                                                              * on the sensor's axis; star participants outside [2^-45, 2^63] */
    uint32_t multi_sector_firings, max_sectors_per_firing, tiles_sectors_fall;
    uint32_t candidates, candidate_cap;   /* entries the scan filed in the march's candidate list (0: no march), the list's length */
    uint32_t reserved[3];
} urf_front_why;                      /* 64 bytes */
int urf_front_explain(urf_ctx* ctx, int layout /* 0 firing order, 1 row-major */, urf_front_why* out /* host */, uint32_t n);

/* ---- urf_set_front_auto: the context applies urf_front_explain's advice itself -----------------------------------
 * One switch for the caller who wants "as fused as my sweeps allow": urf_set_front_mode(ctx, 2); urf_set_front_auto(ctx, 1).  0 (default):
 * as today -- a context that never turns it on allocates and launches nothing for it.  1: below.  Anything else: URF_ERR_INVALID_ARG;
 * URF_ERR_OOM (the pass's buffers, allocated by this call, outside any stream capture): it stays off.
 *
 * WHERE IT ACTS.  In front modes 2 and 3 only, like every other switch: mode 1's batch-size rule is a measured default and stays the
 * caller's decision.  In modes 0 and 1 the switch is remembered and decides nothing (URF_AUTO_IDLE).
 * BITS ARE ONLY EVER ADDED.  Auto turns switches on and raises mode 2 to 3; it never turns anything off.  urf_set_front_auto(ctx, 0) stops
 * it and leaves what it applied: read `applied` and undo by hand what you do not want.  Turning it on again, even when it is on, is a new
 * start.
 * CALL-LEVEL ADVICE is applied at the call itself, on the host, before anything is launched: a batch call and urf_classify_pc2_async ask
 * the policy why the call as it stands would keep the general kernels (urf_front_explain's `call` and `advice`) and apply the advice
 * bits inside URF_ADVICE_AUTO_MASK unless the advice holds NEVER, CAPTURE_OFF or RESET (BATCH does not block: a sweep of the callback
 * path may still be sighted row-major).  The bits go through the setters' own code, allocation included; a setter that answers
 * URF_ERR_OOM puts its bit into `refused`, and the call goes on without it.  The call is then planned once, with the new settings.  (This
 * happens before any scan has been looked at: a switch may be turned on for sweeps that then break a rule no setting lifts.)
 * SCAN-LEVEL ADVICE needs evidence from the device: the learning pass.  While URF_AUTO_LEARNING, a call that launched the fused kernels
 * is followed, on the same stream and inside the same API call, by k_front_explain and k_front_digest
 * (urban_road_filter_amd/csrc/urf_k_front_digest.hpp): eight words in host-mapped memory that the NEXT call reads without waiting -- a
 * digest that has not arrived is looked for again at the call after.  One pass is in flight at a time.  A call that did not launch the
 * fused kernels launches no pass and changes no phase.  The pass reads the call's inputs behind the call's own kernels, in stream order:
 * "the call has completed" already means the pass has, and the LIFETIME contract of the classify calls does not change.  On the callback
 * path the pass runs on the sweep's stream between its launch sequence and the event urf_classify_pc2_wait waits for; it is no part of
 * the captured sequence, a sweep that is voided and run again teaches nothing, and the re-run launches no pass.
 * A digest that has arrived: scans its firings' sectors hand back (digest_helped > 0) while urf_set_front_multi_sector (curbPoints != 5:
 * urf_set_front_multi_sector_curb_points too) is off -> both are applied, still learning.  Otherwise, nothing handed back, or every
 * handed-back scan has a reason no setting lifts (digest_never + digest_candidates == digest_handed_back) -> URF_AUTO_SETTLED.  Otherwise,
 * with OTHER or ROWS_SIGHTING among the bits (CALL_AGAIN: a repaired speculation, a first sighting) -> still learning, at most three
 * times per new start, then settled.  At most five calls per new start carry a pass that counts (explained_calls); on the callback
 * path a sweep that is voided carries one that is discarded and not counted -- once per kind of URF_STATUS_REDO_*, at most.
 * A NEW START (learning again, explained_calls 0, `refused` cleared, `applied` kept): urf_set_params with other parameters,
 * urf_set_front_mode with another mode or ending a sticky read-out, a switch setter that changes its switch, a row-major sighting,
 * urf_set_front_auto(ctx, 1).
 * SETTLED COSTS NOTHING: a settled context launches exactly what a context with the same switches set by hand launches.  It does not
 * look again when the stream changes character: urf_set_front_auto(ctx, 1) starts it over.
 * The sticky read-out (READOUT: RESET, FRONT_OUTPUTS), CAPACITY, BATCH, CAPTURE_OFF and NEVER are reported in `left` and never applied. */
int urf_set_front_auto(urf_ctx* ctx, int on);
#define URF_ADVICE_AUTO_MASK (URF_ADVICE_MODE_3 | URF_ADVICE_LASERS128 | URF_ADVICE_LONG_SWEEPS | URF_ADVICE_CURB_POINTS | \
                              URF_ADVICE_MULTI_SECTOR | URF_ADVICE_MULTI_SECTOR_CP)
#define URF_AUTO_IDLE     0u   /* off, or front mode 0 / 1 */
#define URF_AUTO_LEARNING 1u
#define URF_AUTO_SETTLED  2u
typedef struct urf_front_auto_info {
    uint32_t on, phase;
    uint32_t applied;          /* URF_ADVICE_* bits the context turned on by itself since the switch was first turned on */
    uint32_t refused;          /* bits it tried and could not have (URF_ERR_OOM): left off, not tried again before a new start */
    uint32_t left;             /* advice of the last call / digest that auto never applies (NEVER, CAPACITY, BATCH, CAPTURE_OFF, RESET, FRONT_OUTPUTS, CALL_AGAIN) */
    uint32_t explained_calls;  /* calls behind which the learning pass was launched since the last new start */
    /* the last digest: its sequence number, scans with a result (URF_TOO_FEW_POINTS, an empty scan and a voided sweep count nowhere),
     * those whose flag is cleared, the OR of their URF_WHY_SCAN_* bits, and how many of them have only MULTI_SECTOR / SECTORS_FALL,
     * one of the four shape bits or ROWS_LENGTH, CANDIDATES, OTHER */
    uint32_t digest_seq, digest_scans, digest_handed_back, digest_scan_bits, digest_helped, digest_never, digest_candidates, digest_other;
    uint32_t reserved[2];
} urf_front_auto_info;                /* 64 bytes */
/* Synchronises the context's stream(s), then reports: the digest of a pass that has completed is shown whether or not a call has
 * taken it yet.  Changes nothing.  With the switch off everything but `applied` reads 0. */
int urf_front_auto_query(urf_ctx* ctx, urf_front_auto_info* out);

/* ---- dense sweeps: put back into firing slots by laser id, on the device ---------
 * The fused front end above wants point f * L + l to be laser slot l of firing f (L = channels), non-returns left in place as holes.  A
 * driver that DROPS non-returns (velodyne_pointcloud's default mode, any is_dense cloud) publishes firings of unequal length back to
 * back: lane is no longer laser, and such a sweep keeps the general kernels.  The same drivers write a laser id per point (the `ring`
 * field: UINT16 in Velodyne's PointXYZIR, UINT8 or UINT16 in Ouster's).  These entry points use it to rebuild the holes.
 * THE RULE.  Point i = 0..n-1 of a dense scan has slot s_i < L (its id, through the slot map below).  A firing starts at i = 0 and
 * wherever s_i <= s_{i-1}; f_i = the number of starts up to and including i, minus 1.  The padded scan has W * L points (W =
 * max_firings: what the sensor delivers per revolution, e.g. 1808 or 2048), all NaN, with point i written at f_i * L + s_i.
 * WHY IT IS EXACT.  f_i * L + s_i grows strictly with i (inside a firing the slot grows, a new firing adds L and takes at most L - 1
 * away), so the padded scan holds the dense points in their input order with holes between them.  The reference drops such holes
 * before anything else (ConditionalRemoval, lidar_segmentation.cpp:100-117) and never looks at an input index: its labels at those
 * positions, and its summary counts, are those of the dense scan.  This holds for ANY ids; nothing depends on their being right.
 * Wrong ids cost speed only: the fused front end finds lane != ring and hands the scan back to the general kernels, as it does for any
 * scan without the shape.  (Adjacent short firings whose slots keep growing merge into one; that loses the sector alignment of those
 * points, nothing else.)
 * THE CALLS.  Inputs, offsets, labels and infos exactly as for urf_classify_batch_soa_ragged / urf_classify_batch_pc2_ragged (scan s =
 * [d_offsets[s], d_offsets[s+1]); d_labels and d_info index the DENSE points and scans) and the same bytes come out.  d_laser: one id
 * per point, laid out like d_x, laser_bytes = 1 (uint8) or 2 (uint16); PointCloud2: a little-endian UINT8 / UINT16 at off_laser of
 * every record, any alignment.  W * L > max_points, max_len > W * L or n_scans > max_batch: URF_ERR_CAPACITY; laser_bytes not 1 or 2,
 * off_laser + laser_bytes > point_step or a NULL pointer: URF_ERR_INVALID_ARG; n_scans == 0 is a no-op (max_firings == 0 with scans
 * to classify: URF_ERR_CAPACITY by the rule above, URF_ERR_INVALID_ARG when all of them are empty).  The padded
 * batch (n_scans scans of W * L points in the context's own staging) then goes through the pipeline as a plain batch call:
 * urf_set_front_mode, urf_set_front_lasers128, urf_set_front_long_sweeps, hand-back, sightings and urf_front_scans mean what they mean
 * for urf_classify_batch_soa.  The first dense call allocates what the re-alignment needs (4 + 1 bytes per point of max_points *
 * max_batch next to the SoA staging; URF_ERR_OOM from that call); a context that never makes one allocates and launches nothing new.
 * A SCAN THAT IS NOT ALIGNED -- a slot >= L, an id the map does not hold, or more than W firings -- is no error: its points are
 * written unpadded (point i at position i, NaN behind them) and classified by whichever kernels take it, with the same labels.
 * urf_dense_scans: how many scans of the last dense call were aligned (synchronises, like urf_front_scans).
 * urf_set_dense_slots: the driver's id -> the laser's position inside a firing, n_ids <= 256 entries (Velodyne's `ring` counts by
 * elevation while its lasers fire in laser-number order); NULL: the identity (default).  An id at or beyond n_ids is held by no slot.
 * The map is copied; the next dense call takes it to the device.
 * AFTER A DENSE CALL the context's record of "the last call" is the padded batch, every buffer of it the context's own:
 * urf_marker_points / urf_marker_points_batch work as ever (marker points are coordinates) and need nothing of the caller's kept
 * alive; urf_clouds_batch_soa / urf_clouds_batch_pc2 with URF_ORDER_INPUT read the caller's dense labels and inputs (LIFETIME as
 * above) and give the records the ragged call gives.  urf_ordered_indices*, urf_clouds_batch_* with URF_ORDER_REFERENCE and
 * urf_read_stage would answer in padded indices: they return URF_ERR_INVALID_ARG (urf_last_error says why) and leave the context
 * as it was -- unless urf_set_dense_outputs is on.
 * urf_set_dense_outputs(ctx, 1): after a dense call urf_ordered_indices, urf_ordered_indices_batch and urf_clouds_batch_* with
 * URF_ORDER_REFERENCE answer in the CALLER'S indices.  The padded scan holds the dense points in input order, so the reference's orders
 * on it are the dense scan's with every index i replaced by its padded position; a device pass behind the list kernels
 * (k_dense_inverse once per dense call, k_dense_unmap_lists per read-out) replaces them back.  The lists hold indices 0 .. len_s - 1
 * into dense scan s in the reference's order, the counts are as ever; urf_ordered_indices' host buffers need room for the dense scan's
 * length, urf_ordered_indices_batch's stride must be at least the dense call's max_len (not W * L; smaller: URF_ERR_INVALID_ARG).
 * urf_clouds_batch_* give counts, offsets and records exactly as after urf_classify_batch_*_ragged on the same points (capacity
 * 3 * n_scans * max_len of the dense call): `roi` from the dense labels in input order, the three ordered clouds gathered from the
 * caller's dense inputs through the mapped lists.  LIFETIME: the ordered indices need nothing of the caller's; the reference-order
 * clouds read the caller's dense labels and inputs, as the input-order clouds do.  Scans that were not aligned, empty,
 * URF_TOO_FEW_POINTS or cut at max_len give what the ragged call gives.  Both positions of urf_set_front_outputs work: off, a fused
 * dense call's padded batch is run again through the general kernels (every buffer the context's; the context stays with those), on,
 * there is no second run.  The first such read-out allocates the inverse map (4 bytes per point of max_points * max_batch;
 * URF_ERR_OOM from that read-out, the context keeps working).  The switch itself allocates and launches nothing, decides nothing about
 * which kernels classify, forgets no sighting or hand-back, and decides nothing after a call that was not dense.  0 (default): the
 * refusals above.  Anything else: URF_ERR_INVALID_ARG.
 * urf_read_stage stays refused after a dense call in either position: stage values are defined per PADDED input point and are a
 * parity tool, not a published output.
 * The kernels are urban_road_filter_amd/csrc/urf_k_dense.hpp; they run outside the timing brackets below. */
int urf_classify_batch_soa_dense(urf_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                 const void* d_laser, uint32_t laser_bytes,
                                 const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                 uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info);
int urf_classify_batch_pc2_dense(urf_ctx* ctx, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total,
                                 uint32_t max_len, uint32_t n_scans, uint32_t point_step,
                                 uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                 uint32_t off_laser, uint32_t laser_bytes,
                                 uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info);
int urf_set_dense_slots(urf_ctx* ctx, const uint8_t* slot_of_id, uint32_t n_ids);
int urf_dense_scans(urf_ctx* ctx, uint32_t* n_aligned);
int urf_set_dense_outputs(urf_ctx* ctx, int on);

/* ---- dense sweeps without a `ring` field: laser ids from elevation, on the device ---------
 * The reference subscribes to pcl::PointXYZI -- x, y, z, intensity, no `ring` --, and a dense cloud of that kind has no id to hand to
 * the calls above.  These calls derive one per point from its vertical angle and then run the dense calls unchanged.
 * THE ID RULE.  The caller states once per context the elevation in degrees of the laser in every slot of a firing: elev_deg[l],
 * l = 0 .. n-1, in firing order (the order urf_set_dense_slots maps to; the sensor's datasheet has the table).  On the host the slots
 * are ranked by ascending elevation, the lower slot first among equals: e_0 <= ... <= e_{n-1}, slot_of_rank[n], and for k = 0 .. n-2
 * T[k] = (float)tan((e_k + e_{k+1}) / 2 * pi / 180), computed in double.  On the device, per point: h = sqrtf(x * x + y * y); rank =
 * the number of k with z > T[k] * h; id = slot_of_rank[rank].  T[k] * h does not decrease with k for h >= 0, so the rank is a binary
 * search of at most 7 steps.
 * EDGE POINTS get whatever the compares give: a point with a NaN field, a point at (0, 0, 0) or a point on the sensor's axis has rank
 * 0, or n-1 for z > 0 on the axis (infinite fields: as IEEE multiplies and compares them); a point outside the sensor's fan takes the
 * outermost laser's slot; two lasers of equal elevation cannot be told apart (the lower slot ranks first, the threshold between them
 * is their own tangent, and their points fall to either side of it).  All of this costs speed only: by THE RULE above, labels and
 * summaries are those of the ragged call for any ids whatever, and a scan whose derived ids do not line up is "not aligned" or handed
 * back like any other.
 * urf_set_dense_elevations: n = 1 .. 128 values, each finite and strictly inside (-90, 90); anything else: URF_ERR_INVALID_ARG, and
 * the table set before stays.  NULL with n = 0 clears it.  The table is copied; the next elevation call takes it to the device.
 * THE CALLS.  urf_classify_batch_soa_dense / urf_classify_batch_pc2_dense without d_laser / off_laser and laser_bytes: every argument
 * rule, capacity rule, "not aligned" rule and everything under AFTER A DENSE CALL holds as written there (urf_dense_scans,
 * urf_front_scans, urf_set_dense_outputs and the read-outs, urf_read_stage's refusal).  Added: no table set, or a table whose n is
 * not the parameters' `channels` at the call: URF_ERR_INVALID_ARG, urf_last_error says which.  The derived ids are slots: the map of
 * urf_set_dense_slots does not apply to them and is left as it is for the next call with ids of the caller's.  The first such call
 * allocates one byte per point of max_points * max_batch for the ids (URF_ERR_OOM from that call), which are kept at the indices of
 * the caller's arrays: urf_classify_batch_soa_dense_elev therefore wants d_offsets[n_scans] <= max_points * max_batch, as
 * urf_classify_batch_pc2_dense_elev checks of n_total (the offsets live on the device, the call cannot answer URF_ERR_CAPACITY for
 * them; ids beyond that are not written).  A context that never makes such a call allocates and launches nothing new.
 * The kernels (k_dense_ids_soa / k_dense_ids_pc2, urf_k_dense.hpp) run in front of the dense calls', outside the timing brackets. */
int urf_set_dense_elevations(urf_ctx* ctx, const float* elev_deg, uint32_t n);
int urf_classify_batch_soa_dense_elev(urf_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                      const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans,
                                      uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info);
int urf_classify_batch_pc2_dense_elev(urf_ctx* ctx, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total,
                                      uint32_t max_len, uint32_t n_scans, uint32_t point_step,
                                      uint32_t off_x, uint32_t off_y, uint32_t off_z,
                                      uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info);

/* ---- per-kernel timing (benchmark) ------------------------------------------
 * With timing on, every classify call brackets each kernel of the pipeline
 * with hipEvents on the context's stream.  urf_kernel_timing() synchronises,
 * adds the elapsed milliseconds of all calls since the last query to
 * ms_sum[0..URF_NUM_KERNELS) and the number of calls to *n_calls, then resets. */
#define URF_NUM_KERNELS 8
int urf_enable_kernel_timing(urf_ctx* ctx, int on);
int urf_kernel_timing(urf_ctx* ctx, double* ms_sum, uint32_t* n_calls);
const char* urf_kernel_name(int index);

/* ---- diagnostics --------------------------------------------------------- */
/* The cotangent (of an angle in degrees, clamped to [1, 179]) from which k_ring_table derives the
 * thresholds on u = -z / rho that decide a point's ring: the same source evaluated on the host, so that
 * its accuracy (1e-15; needed: 1e-7) can be checked without a GPU. */
double urf_ring_threshold_cot(double angle_deg);
/* The host-side gather of the callback path by itself (no context, no device): x / y / z of a PointCloud2-layout
 * message into three arrays of n_points floats.  urf_classify_pc2_async() does this into pinned memory with every
 * message it has to stage (12 bytes per point then cross PCIe, whatever the point_step); records whose x, y, z lie
 * side by side with a fourth word behind them inside the record go four at a time through a 4 x 4 transpose. */
int urf_pc2_to_planes(const uint8_t* data, uint32_t n_points, uint32_t point_step, uint32_t off_x, uint32_t off_y,
                      uint32_t off_z, float* x, float* y, float* z);
/* Diagnostics of the callback path.  It launches a short kernel sequence first (no repair kernels behind the
 * speculative ring table, none for the work lists of star sectors of more than 384 points, none for rings that hold a
 * point with a NaN azimuth, none for star sectors with equal planar ranges); a sweep that needed what
 * was left out is run again inside urf_classify_pc2_wait() with the full sequence, and so is every later one.
 * n_rerun: sweeps run again so far (per cause the first one and those in flight beside it); sequence: bit 0 the ring table is still speculative,
 * bit 1 the work-list kernels are part of the sequence, bit 2 so is the kernel for rings with NaN azimuths, bit 3 the ring table also
 * stops at the ring count of the previous sweep (a stream of sweeps from one sensor shows the same rings), bit 4 the kernel that orders
 * equal planar ranges of a star sector as std::sort does is part of the sequence (a real sensor's first sweep switches it on).
 * A stream from a real sensor therefore pays one sweep run twice at its start (and the sweeps in flight beside it) and two more
 * near-empty launches per sweep from then on: bench.py's e2e_latency_ms_sensor_like is that steady state, e2e_latency_ms the
 * tie-free one.
 * Either pointer may be NULL. */
int urf_callback_path_state(const urf_ctx* ctx, uint32_t* n_rerun, uint32_t* sequence);
/* Puts kernels into the callback path's sequence before a sweep has asked for them: sequence_bits = 2 (work lists of large star
 * sectors) | 4 (rings with NaN azimuths) | 16 (std::sort's order of equal planar ranges) -- a node that knows its sensor (every real
 * one delivers equal ranges) calls it with 16 once and saves the stream's first sweeps their second run.  Bits are only ever added. */
int urf_callback_path_preset(urf_ctx* ctx, uint32_t sequence_bits);
const char* urf_strerror(int status);
const char* urf_last_error(const urf_ctx* ctx);   /* text of the last HIP failure */
int urf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* URF_H */
