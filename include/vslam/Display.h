// Drop-in for the reference's include/Display.h without a window: the same DisplayState and a Display with the reference's
// constructor, `ds` member and initialize / close / join, so that src/vslam.cpp compiles -- but no thread is started and
// nothing is shown.  run() (a Pangolin loop) is replaced by render(): `ds` drawn ONCE into an image by the device renderer
// (vslam_render_points, include/vslam_amd.h "the view of the map": points as squares of their colour, one wire frustum per
// frame as draw_box draws it).  Interactive windows, Handler3D and the imshow overlay are out of scope.
#pragma once
#include <mutex>
#include <vector>

#include "../vslam_amd.h"
#include "Frame.h"
#include "PointMap.h"
#include "cvlite.h"
#include "vslam_internal.h"

struct DisplayState {   // reference: include/Display.h:12-17
    cv::Mat *points = NULL;
    usize size = 0;
    std::vector<Frame> *frames = NULL;
    std::vector<cv::Point3_<u8>> *colors = NULL;
};

class Display {
   public:
    // reference: include/Display.h:22.  `view` starts as vslam_view_default(W, H): the reference's camera (src/display.cpp:25-26).
    Display(const char *window_name, const int W, const int H, std::mutex *mtx);
    DisplayState ds;
    vslam_view view;   // set view.flags |= VSLAM_RENDER_AS_REFERENCE for what draw_points_colors actually submits

    void initialize() {}   // the reference opens the window and starts run() in a thread (src/display.cpp:11-18)
    void close() {}
    void join() {}

    // Draws `ds` once, under the mutex as run() reads it (src/display.cpp:39-57): rows 0 .. ds.size - 1 of *ds.points
    // (N x 4 CV_32F, continuous) with (*ds.colors)[i] -- (0, 0, 0) past the end of colors -- and one frustum per frame of
    // *ds.frames whose pose is a continuous 4 x 4 CV_32F (draw_box returns early otherwise).  bgr_out: H x W CV_8UC3.
    // Waits for the device.
    void render(cv::Mat &bgr_out);

   private:
    std::mutex *mtx;
    const char *window_name;
    const int W, H;
};

namespace vslam {
// A map that lives on the device (vslam::map_create / vslam::map_step), seen through `view`: vslam_map_render of its one
// track, copied to the host as an H x W CV_8UC3 image.  Nothing of the map is copied.  Waits for the device.
cv::Mat render_map(PointMap &pm, const vslam_view &view, int W, int H);
}  // namespace vslam
