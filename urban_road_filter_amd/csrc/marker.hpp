/*
 * marker.hpp -- the road_marker MarkerArray of the reference, built on the host from the marker
 * points the GPU finds (urf_marker_points): colour fix-ups, green/red line strips, Douglas-Peucker
 * simplification, polygon height, deletion of obsolete markers
 * (src/lidar_segmentation.cpp:369-602).  Pure host C++, at most 361 points per sweep.  buildMarkerStrips is the one host
 * implementation: urf_marker_strips (include/urf.h) is its C view, MarkerBuilder widens its records to a MarkerArray; the batch
 * form runs on the device (urf_marker_strips_batch, urf_k_markers.hpp) and gives the same records.
 *
 * visualization_msgs::Marker / MarkerArray are mirrored with the members the reference sets.
 * boost::geometry::simplify (third party, not in the reference checkout nor in this image) is
 * restated as Douglas-Peucker with the point-to-segment distance, float coordinates, "keep iff
 * strictly farther than the tolerance"; the real library cannot be run here, the step is pinned by
 * the worked example of Boost.Geometry's documentation and hand-derived cases (urf_simplify_line).
 */
#ifndef URF_MARKER_HPP
#define URF_MARKER_HPP

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "urf.h"

namespace urf {

struct Error : std::runtime_error {
    int code;   /* urf_status */
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

struct Marker {
    enum { LINE_STRIP = 4, ADD = 0, DELETE = 2 };
    std::string frame_id;          /* header.frame_id = params::fixedFrame (:424) */
    int32_t type = LINE_STRIP, action = ADD, id = 0;
    std::array<double, 3> position{ { 0, 0, 0 } };
    std::array<double, 4> orientation{ { 0, 0, 0, 1 } };   /* x y z w (:31-34) */
    std::array<double, 3> scale{ { 0.5, 0.5, 0.5 } };      /* :36-38 */
    std::array<float, 4> color{ { 0, 0, 0, 0 } };           /* r g b a */
    std::vector<std::array<double, 3>> points;
};
struct MarkerArray {
    std::vector<Marker> markers;
};

/* One sweep: the records and packed points of urf_marker_strips (include/urf.h), same arguments and return value. */
int buildMarkerStrips(const float* pts, uint32_t k, const urf_marker_params& mp, int32_t* ghostcount, int32_t* published,
                      urf_marker_strip* strips, uint32_t* n_strips, float* xyz, uint32_t* n_points);
/* ... widened to the message: floats to double, header.frame_id, type, scale and orientation as the reference sets them */
void toMarkerArray(const urf_marker_strip* strips, uint32_t n_strips, const float* xyz, const std::string& fixed_frame, MarkerArray& out);

/* Keeps what the reference keeps between callbacks: ghostcount (lidar_segmentation.cpp:23).  The reference's member
 * linestring (data_structures.hpp:139) is always empty between sweeps (marker colours are 0 / 1: DESIGN.md section 4). */
class MarkerBuilder {
public:
    MarkerBuilder();
    void setParams(const urf_marker_params& p) { params_ = p; }
    void setFixedFrame(const std::string& f) { fixed_frame_ = f; }
    /* pts: k x {x, y, z, red} from urf_marker_points.  Returns false when the reference would
     * publish no MarkerArray for this sweep (fewer than 3 marker points, :371).  Input urf_marker_points cannot give
     * (k > 361, a colour other than 0 / 1) throws Error(URF_ERR_INVALID_ARG).
     * Nothing is allocated per sweep beyond what `out` grows to. */
    bool build(const float* pts, uint32_t k, MarkerArray& out);
    void reset() { ghostcount_ = 0; }
    int32_t ghostcount() const { return ghostcount_; }

private:
    urf_marker_params params_;
    std::string fixed_frame_;
    int32_t ghostcount_ = 0;
};

/* Douglas-Peucker on float points; returns the kept points in order. */
std::vector<std::array<float, 2>> simplifyLine(const std::vector<std::array<float, 2>>& line, float tolerance);

}   // namespace urf
#endif
