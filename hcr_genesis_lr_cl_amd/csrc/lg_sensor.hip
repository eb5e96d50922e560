// lg_sensor.hip -- the depth camera behind include/lgsensor.h: one ray per pixel against the heightfield the physics stands on.
//
// Reference call sites replaced: genesis_simulator.py:803-819 (gs.sensors.DepthCamera mounted on the base) and :741-750 (read, clip,
// normalise).  The surface is terrain_at's (lg_kernel.h): inside grid cell (i, j) the bilinear patch of its four corners; reading the
// corners through an index clamped to the grid reproduces terrain_at's clamped index / fraction outside it.  Along a ray
// z(t) - h(x(t), y(t)) is a quadratic in t inside one cell, so the kernel walks the cells the ray's ground track crosses (2-D DDA from
// the camera origin) and takes the first root inside each cell's [t_enter, t_exit].
//
// This is a latency-bound gather: a handful of int16 loads per cell out of a heightfield that sits in L2, ~30 flops between them.
// One pixel per lane; the 256 pixels of a workgroup belong to one env, so the pose, the composed rotation and every scene constant are
// wave-uniform (SGPRs) and a wave's 64 stores are 256 contiguous bytes.  No LDS, no scratch, many waves per SIMD.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include "../../include/lgsensor.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

#define DEPTH_BLOCK 256

struct DepthArgs {
    LgDepthCam cam; LgDepthScene sc; const float *dirs; float *out;
    int n_pix, blocks_per_env, cap;
};

// rotation matrix of a unit quaternion (xyzw), row-major
static __device__ __forceinline__ void quat_matrix(float x, float y, float z, float w, float R[9]) {
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z); R[2] = 2.f * (x * z + w * y);
    R[3] = 2.f * (x * y + w * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
    R[6] = 2.f * (x * z - w * y); R[7] = 2.f * (y * z + w * x); R[8] = 1.f - 2.f * (x * x + y * y);
}

// heightfield corner with the index clamped to the grid: always inside the allocation
static __device__ __forceinline__ float corner(const int16_t *__restrict__ hf, int i, int j, int rows, int cols, float vscale) {
    i = min(max(i, 0), rows - 1);
    j = min(max(j, 0), cols - 1);
    return (float)hf[(size_t)i * cols + j] * vscale;
}

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_render_kernel(DepthArgs a) {
    const int env = blockIdx.x / a.blocks_per_env;                                   // wave-uniform
    const int pix = (blockIdx.x - env * a.blocks_per_env) * DEPTH_BLOCK + threadIdx.x;
    if (pix >= a.n_pix) return;
    const float *bp = a.sc.base_pos + 3 * (size_t)env, *bq = a.sc.base_quat + 4 * (size_t)env;
    float Rb[9], Rm[9], M[9];
    quat_matrix(bq[0], bq[1], bq[2], bq[3], Rb);
    quat_matrix(a.cam.mount_quat[0], a.cam.mount_quat[1], a.cam.mount_quat[2], a.cam.mount_quat[3], Rm);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[3 * r + c] = Rb[3 * r] * Rm[c] + Rb[3 * r + 1] * Rm[3 + c] + Rb[3 * r + 2] * Rm[6 + c];
    const float mx = a.cam.mount_pos[0], my = a.cam.mount_pos[1], mz = a.cam.mount_pos[2];
    const float ox = bp[0] + Rb[0] * mx + Rb[1] * my + Rb[2] * mz;
    const float oy = bp[1] + Rb[3] * mx + Rb[4] * my + Rb[5] * mz;
    const float oz = bp[2] + Rb[6] * mx + Rb[7] * my + Rb[8] * mz;
    const float *rd = a.dirs + 3 * (size_t)pix;
    const float cx = rd[0], cy = rd[1], cz = rd[2];
    const float dx = M[0] * cx + M[1] * cy + M[2] * cz;
    const float dy = M[3] * cx + M[4] * cy + M[5] * cz;
    const float dz = M[6] * cx + M[7] * cy + M[8] * cz;
    const float max_range = a.cam.max_range;
    float hit = INFINITY;
    const bool finite = isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(dx) && isfinite(dy) && isfinite(dz);
    if (finite && a.sc.rows == 0) {                                                  // the plane z = 0
        if (oz <= 0.f) hit = 0.f;
        else if (dz < 0.f) hit = -oz / dz;
    } else if (finite) {
        const int rows = a.sc.rows, cols = a.sc.cols;
        const float hs = a.sc.hscale, vs = a.sc.vscale;
        const int16_t *__restrict__ hf = a.sc.heightfield;
        // grid coordinates of the origin as terrain_at forms them; everything after is relative to the origin's cell
        const float gx0 = (ox + a.sc.border) / hs, gy0 = (oy + a.sc.border) / hs;
        const float flx = fminf(fmaxf(floorf(gx0), -1.0e9f), 1.0e9f), fly = fminf(fmaxf(floorf(gy0), -1.0e9f), 1.0e9f);
        const int i0 = (int)flx, j0 = (int)fly;
        const float fx0 = fminf(fmaxf(gx0 - flx, 0.f), 1.f), fy0 = fminf(fmaxf(gy0 - fly, 0.f), 1.f);
        const float dgx = dx / hs, dgy = dy / hs;                                    // grid cells per metre of range
        const float inv_x = 1.f / dgx, inv_y = 1.f / dgy;
        const int sx = dgx > 0.f ? 1 : -1, sy = dgy > 0.f ? 1 : -1;
        const int px = dgx > 0.f ? 1 : 0, py = dgy > 0.f ? 1 : 0;
        int di = 0, dj = 0;
        float t_enter = 0.f;
        for (int it = 0; it < a.cap; it++) {                                         // the cap bounds the walk whatever the input
            const float tx = dgx != 0.f ? ((float)(di + px) - fx0) * inv_x : INFINITY;
            const float ty = dgy != 0.f ? ((float)(dj + py) - fy0) * inv_y : INFINITY;
            const float t_exit = fminf(fminf(tx, ty), max_range);
            const float z0 = oz + t_enter * dz, z1 = oz + t_exit * dz;
            const int i = i0 + di, j = j0 + dj;
            const float h00 = corner(hf, i, j, rows, cols, vs), h10 = corner(hf, i + 1, j, rows, cols, vs);
            const float h01 = corner(hf, i, j + 1, rows, cols, vs), h11 = corner(hf, i + 1, j + 1, rows, cols, vs);
            if (!(fminf(z0, z1) > fmaxf(fmaxf(h00, h10), fmaxf(h01, h11)))) {        // else the ray stays above the whole patch
                const float u0 = fminf(fmaxf(fx0 + t_enter * dgx - (float)di, 0.f), 1.f);
                const float v0 = fminf(fmaxf(fy0 + t_enter * dgy - (float)dj, 0.f), 1.f);
                const float b = h10 - h00, c = h01 - h00, e = (h11 - h01) - b;
                // g(s) = z - h along the ray from the cell entry, s = t - t_enter: C + B s + A s^2
                const float C = z0 - (h00 + b * u0 + c * v0 + e * u0 * v0);
                if (C <= 0.f) { hit = t_enter; break; }                              // entered at or below the surface
                const float B = dz - b * dgx - c * dgy - e * (u0 * dgy + v0 * dgx);
                const float A = -e * dgx * dgy;
                const float disc = B * B - 4.f * A * C;
                if (disc >= 0.f) {
                    const float q = -0.5f * (B + copysignf(sqrtf(disc), B));
                    const float r1 = q / A, r2 = C / q, S = t_exit - t_enter;        // A == 0 or q == 0: inf / NaN fail the tests below
                    float s = INFINITY;
                    if (r1 > 0.f && r1 <= S) s = r1;
                    if (r2 > 0.f && r2 <= S && r2 < s) s = r2;
                    if (s < INFINITY) { hit = t_enter + s; break; }
                }
            }
            if (!(t_exit < max_range)) break;
            if (tx <= ty) di += sx; else dj += sy;
            t_enter = t_exit;
        }
    }
    float v = hit < max_range ? hit : max_range;
    v = fmaxf(v, a.cam.min_range);
    if (a.cam.normalize) {                                                           // genesis_simulator.py:745-750
        const float near_clip = a.cam.near_clip, far_clip = a.cam.far_clip;
        v = (fminf(fmaxf(v, near_clip), far_clip) - near_clip) / (far_clip - near_clip) - 0.5f;
    }
    a.out[(size_t)env * a.n_pix + pix] = v;
}

extern "C" int lg_depth_render(const LgDepthCam *cam, const LgDepthScene *scene, const float *ray_dirs, float *out, void *stream) {
    if (!cam || !scene || !ray_dirs || !out) return lg_fail_msg("lg_depth_render: null argument");
    if (!scene->base_pos || !scene->base_quat) return lg_fail_msg("lg_depth_render: null base pose");
    if (cam->width < 1 || cam->height < 1 || scene->n_envs < 1) return lg_fail_msg("lg_depth_render: non-positive size");
    if (!(cam->max_range > cam->min_range) || !(cam->min_range >= 0.f) || !isfinite(cam->max_range))
        return lg_fail_msg("lg_depth_render: need 0 <= min_range < max_range, finite");
    if (!(cam->far_clip > cam->near_clip) || !isfinite(cam->far_clip) || !isfinite(cam->near_clip))
        return lg_fail_msg("lg_depth_render: need near_clip < far_clip, finite");
    int cap = 0;
    if (scene->rows != 0) {
        if (scene->rows < 2 || scene->cols < 2 || !scene->heightfield) return lg_fail_msg("lg_depth_render: a heightfield needs at least 2 x 2 samples and a pointer");
        if (!(scene->hscale > 0.f) || !isfinite(scene->vscale) || !isfinite(scene->border)) return lg_fail_msg("lg_depth_render: bad heightfield scales");
        const float cells = cam->max_range / scene->hscale;
        if (!(cells <= (float)LG_DEPTH_MAX_CELLS)) return lg_fail_msg("lg_depth_render: max_range / hscale exceeds LG_DEPTH_MAX_CELLS");
        cap = 2 * (int)ceilf(cells) + 4;      // the ground track crosses at most sqrt(2) * max_range / hscale + 2 cell borders
    }
    const long long n_pix = (long long)cam->width * cam->height;
    const long long bpe = (n_pix + DEPTH_BLOCK - 1) / DEPTH_BLOCK;
    if (n_pix * scene->n_envs >= (1ll << 31) || bpe * scene->n_envs >= (1ll << 31)) return lg_fail_msg("lg_depth_render: 2^31 pixels or more");
    DepthArgs a;
    a.cam = *cam; a.sc = *scene; a.dirs = ray_dirs; a.out = out;
    a.n_pix = (int)n_pix; a.blocks_per_env = (int)bpe; a.cap = cap;
    hipLaunchKernelGGL(depth_render_kernel, dim3((unsigned)(bpe * scene->n_envs)), dim3(DEPTH_BLOCK), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return lg_fail_msg(std::string("lg_depth_render: ") + hipGetErrorString(e));
    return 0;
}
