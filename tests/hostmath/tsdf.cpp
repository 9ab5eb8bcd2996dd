// Host build of csrc/tsdf_math.h for tests/test_tsdf_cpu.py: the pixel and the observation of a (corner, camera) pair, the
// sphere test and the unprojection of a pixel position that the kernels of csrc/tsdf.hip call, behind a C interface
// (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/tsdf_math.h"

extern "C" {

int32_t th_camera_bytes() { return (int32_t)sizeof(ts_tsdf_camera); }
int64_t th_pixel(const ts_tsdf_camera* cam, float x, float y, float z, float znear, float* z_out) {
    const float p[3] = {x, y, z};
    return ts_tsdf_pixel(*cam, p, znear, z_out);
}
int32_t th_observe(float d, float z, float trunc, float depth_max, float* t) {
    return ts_tsdf_observe(d, z, trunc, depth_max, t) ? 1 : 0;
}
int32_t th_cull(const ts_tsdf_camera* cam, float cx, float cy, float cz, float radius, float znear) {
    const float c[3] = {cx, cy, cz};
    return ts_tsdf_cull(*cam, c, radius, znear) ? 1 : 0;
}
int32_t th_unproject(const ts_tsdf_camera* cam, double u, double v, double z, double* out) {
    return ts_tsdf_unproject(*cam, u, v, z, out) ? 1 : 0;
}

}  // extern "C"
