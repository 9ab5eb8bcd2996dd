// Host build of csrc/depth_prior_math.h for tests/test_depth_prior_cpu.py: the projection of a point, the sort key, the
// sampling of a dense map, the order-preserving image of a double and the target's arithmetic that the kernels of
// csrc/depth_prior.hip call, behind a C interface (compiled with -ffp-contract=off, as the kernels are).
#include "../../tinysplat_amd/csrc/depth_prior_math.h"

extern "C" {

int64_t dh_project(const float* cam, int32_t width, int32_t height, float x, float y, float z, double error, float* z_out) {
    return ts_depth_project(cam, width, height, x, y, z, error, z_out);
}
int64_t dh_no_pixel() { return TS_DEPTH_NO_PIXEL; }
int64_t dh_key(int32_t camera, int64_t pixel, int32_t position) { return ts_depth_key(camera, pixel, position); }
int64_t dh_key_pixel(int64_t key) { return ts_depth_key_pixel(key); }
int32_t dh_key_camera(int64_t key) { return ts_depth_key_camera(key); }
int64_t dh_key_run(int64_t key) { return ts_depth_key_run(key); }
float dh_sample(const float* map, int32_t h, int32_t w, int32_t height, int32_t width, int32_t u, int32_t v) {
    return ts_depth_sample_dense(map, h, w, height, width, u, v);
}
uint64_t dh_order_key(double r) { return ts_depth_order_key(r); }
double dh_order_value(uint64_t k) { return ts_depth_order_value(k); }
float dh_apply(double s, double t, float dense, int32_t disparity) { return ts_depth_apply(s, t, dense, disparity); }

}  // extern "C"
