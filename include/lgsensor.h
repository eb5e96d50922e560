/* lgsensor.h -- C ABI of the exteroceptive sensors: a depth camera that ray-casts the terrain the robots stand on
 * (the reference's genesis_simulator.py:803-819 mounts a gs.sensors.DepthCamera on the robot, :741-750 reads and normalises it).
 * Same conventions as lgrollout.h: plain device pointers, sizes, the caller's HIP stream as void*; 0 on success, otherwise non-zero
 * with the message in lgsim.h's last-error call.  No handle: every call carries the whole scene.
 */
#ifndef LGSENSOR_H
#define LGSENSOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* max_range / hscale above which a render is refused: the cell walk's iteration cap follows from that ratio */
#define LG_DEPTH_MAX_CELLS 4096

/* The camera: a pinhole of width x height pixels mounted on the base.  The camera frame is x forward, y left, z up. */
typedef struct LgDepthCam {
    int32_t width, height;
    float mount_pos[3];    /* camera origin in the base frame, m */
    float mount_quat[4];   /* camera frame -> base frame, xyzw, unit */
    float min_range;       /* the reported range is clamped to [min_range, max_range]; no hit gives max_range */
    float max_range;
    float near_clip;       /* normalize != 0: out = (clip(range, near_clip, far_clip) - near_clip) / (far_clip - near_clip) - 0.5 */
    float far_clip;
    int32_t normalize;
} LgDepthCam;

/* The scene: the base poses and the int16 heightfield the engine was given (rows x cols, row-major, height = sample * vscale at
 * world (row * hscale - border, col * hscale - border)).  rows == 0 is the plane z = 0. */
typedef struct LgDepthScene {
    int32_t n_envs;
    const float *base_pos;        /* (N, 3) */
    const float *base_quat;       /* (N, 4) xyzw, unit */
    const int16_t *heightfield;   /* may be NULL when rows == 0 */
    int32_t rows, cols;
    float hscale, vscale, border;
} LgDepthScene;

/* One range image per env in ONE launch: out (N, height, width) float32 row-major, pixel row 0 at the top, column 0 at the left.
 * ray_dirs: device table (height * width, 3) of unit directions in the camera frame, the pixels in the same row-major order.
 * The surface is the one the physics stands on: inside grid cell (i, j) the bilinear patch of its four corners, with the corner
 * index clamped to the grid (so the outermost samples extend to infinity).  The value is the distance along the ray to its first
 * point at or below the surface, clamped to [min_range, max_range]; an origin at or below the surface gives min_range; a non-finite
 * pose or direction gives max_range.  The cell walk is capped at 2 * ceil(max_range / hscale) + 4 cells.
 * Refused before the launch: a null pointer, a non-positive size, max_range <= min_range, far_clip <= near_clip, rows == 1 or
 * cols < 2 with rows > 0, a non-positive hscale with rows > 0, max_range / hscale > LG_DEPTH_MAX_CELLS, an image of 2^31 pixels or
 * more. */
int lg_depth_render(const LgDepthCam *cam, const LgDepthScene *scene, const float *ray_dirs, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGSENSOR_H */
