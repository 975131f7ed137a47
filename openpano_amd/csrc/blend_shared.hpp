// blend_shared.hpp -- what the host-only units of the blend stage (blend_geom.cc, photometric_solve.cc: plain C++, no HIP) share
// with its device units (blend.hip, overlap.hip, canvas.hip): the layout of the overlap statistics, the limits of the entry
// points, and the helpers that cross a translation unit.
#pragma once
#include <stdint.h>
#include "op_base.hpp"

#ifdef __HIPCC__
#define OP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define OP_HOST_DEVICE inline
#endif

// pair (a < b) of n images (include/openpano_hip.h)
OP_HOST_DEVICE long long pair_index(int a, int b, int n) { return (long long)a * n - (long long)a * (a + 1) / 2 + (b - a - 1); }

constexpr double GAIN_FIX = 4294967296.0;       // 2^32: the fixed point of every overlap sum
constexpr int GAIN_MAX_BLOCKS = 16;                           // bx, by in [1, 16]
constexpr long long GAIN_BLOCK_MAX_ENTRIES = 1ll << 22;    // P * B^2 (include/openpano_hip.h)
constexpr long long GAIN_BLOCK_MAX_UNKNOWNS = 4096;        // n * B, op_gain_block_solve's dense Cholesky
constexpr int VIG_MOMENTS = 30;                 // moments of a pair (overlap.hip, k_vignette_overlap)

struct BlurTaps { int center; float k[2 * OP_MAX_KCENTER + 1]; };
struct CylProj { double cx, cy; int r, sizefactor; };

// blend_geom.cc
void roi_of(const op_blend_geom* g, const double* range, int roi[4]);
int gauss_taps(float sigma, int window_factor, BlurTaps& t);
CylProj cyl_projector(int w, int h, double h_factor, float focal_length);
int reproject_check(const op_pano_frame* f, const op_view_spec* s);      // op_canvas_reproject's refusals (OP_OK or OP_ERR_INVALID)
// photometric_solve.cc
bool vignette_curve_positive(const double a[3]);
int check_lens_frame(const char* who, const op_blend_image* imgs, int n);
int check_gains(const char* who, const float* gains, long long count, long long per_image);
