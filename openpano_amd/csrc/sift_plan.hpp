// sift_plan.hpp -- the plan of one SIFT batch: working and octave sizes, the workspace layout, the Gaussian bank and the
// scale-space kernel's work split.  sift_plan.cc (plain C++, no HIP) computes it from an op_config and three integers; the
// kernels and sift_host.hip read it through internal.hpp; tests/harness runs build_plan on the CPU under the sanitizers.
#pragma once
#include "op_base.hpp"       // OP_MAX_KCENTER

#ifdef __HIPCC__
#define OP_PLAN_FN __host__ __device__ inline
#else
#define OP_PLAN_FN inline
#endif

#define OP_MAX_OCT 8
#define OP_MAX_SCALE 12      // NUM_SCALE <= 12

// ---------------------------------------------------------------------------------------
// HBM layout of one image's scale space ("image workspace", ws_stride floats per image):
//   for each octave o:  [G 0 = grey][G 1 .. G ns-1]   each h_o*w_o fp32, row-major, octave blocks back to back
// -- the reference's Gaussian stack (feature/dog.cc:53-57: data[0] is the unblurred grey image) and NOTHING else.
// The DoG planes (dog.cc:116-129) are never materialised: the extrema scan runs on them while they are in LDS
// (pyramid.hip), and the sub-pixel refinement -- the only other reader, a few hundred sparse 3x3x3 neighbourhoods per
// image -- evaluates |G[l] - G[l+1]| (dog.cc:126) on the two Gaussian planes, the same fp32 operation on the same
// operands: 28 bytes per octave pixel cross the HBM boundary in the scale-space kernel instead of 44.  The mag/ort
// planes of GaussianPyramid::cal_mag_ort (dog.cc:60-94) are not materialised either -- the orientation and
// descriptor kernels evaluate the same expressions on the Gaussian plane for exactly the window samples they use.
// ---------------------------------------------------------------------------------------
struct OctDesc {
	int h, w;
	int tiles_x, tiles_y, tile_begin;   // pyramid-kernel tiling (k_pyramid)
	int rw_nb, rw_nseg;                 // k_pyramid_rows: bands x row segments of this octave
	long long off;                      // float offset of the octave block in the image workspace
	long long plane;                    // h*w
};

struct SiftPlan {
	int n;                      // images in the batch (all sh x sw)
	int sh, sw;                 // source size
	int wh, ww;                 // working size (feature.cc:33-35)
	int noct, nscale;
	OctDesc oct[OP_MAX_OCT];
	int total_tiles;
	long long ws_stride;        // floats per image workspace
	float* ws;
	float* work;                // n x wh x ww x 3 (only materialised for the staged dump)
	const void* const* srcs;    // device array of n source pointers (device memory)
	int src_u8;                 // 0: fp32 sources, 1: uint8 sources (converted like read_img, lib/imgio.cc:54-56)
	int* zero;                  // batch counters cleared by the first kernel of the step (k_grey_octaves), zero_n ints
	int zero_n;
	int num_cu;                 // compute units of the device
	// Gaussian bank (feature/gaussian.cc:17-40): kern[s][center + k], s = 1..nscale-1
	float kern[OP_MAX_SCALE][2 * OP_MAX_KCENTER + 1];
	int kcenter[OP_MAX_SCALE];
	int halo;                   // max kcenter
	// Row-streaming scale-space kernel (k_pyramid_rows): available when the bank is the shipped one
	// (7 scales, half-widths 3,3,3,6,6,6).  kpair[pl][d] = taps at distance d from the centre of the
	// two sigmas (2 pl + 1, 2 pl + 2) that share one packed accumulator; a shorter kernel is
	// zero-extended (adding +-0 leaves an fp32 sum unchanged, so the padding is exact).
	int rows_ok;
	int rw_seg;                 // rows of a segment (chosen per batch: the launch should be a whole number of device fills, sift_plan.cc)
	int rw_items;               // work items per image: sum over octaves of bands x segments
	float kpair[3][7][2];
	// thresholds
	float pre_color_thres, judge_thres, contrast_thres, edge_ratio, offset_thres;
	int calc_offset_depth;
	float gauss_sigma, scale_factor, ori_radius;
	int ori_smooth, desc_scale_factor, desc_int_factor;
	int desc_list_cap;          // k_descriptor: floats of list arena one sorting pass may use (the arena's size; a test lowers it to force the two-pass path)
};

OP_PLAN_FN long long plane_off_grey(const OctDesc& o) { return o.off; }
OP_PLAN_FN long long plane_off_gauss(const OctDesc& o, int ns, int s) { (void)ns; return o.off + (long long)s * o.plane; }   // s = 0: grey
OP_PLAN_FN int planes_per_octave(int ns) { return ns; }

#define OP_DESC_LIST_CAP 640   // k_descriptor: floats in the list arena of one batch's counting sort
#define OP_RW_OWN 240     // k_pyramid_rows: columns owned by a band
// rows of a segment: chosen per batch between OP_RW_SEG_MIN and OP_RW_SEG_MAX (build_plan's pin_seg pins it: a build of
// sift_host.hip with -DOP_RW_SEG=<rows> passes it, for A/B runs)
#define OP_RW_SEG_DEFAULT 24
#define OP_RW_SEG_MIN 16
#define OP_RW_SEG_MAX 40
#define OP_PYR_TW 64
#ifndef OP_PYR_TH
#define OP_PYR_TH 16
#endif

// The plan of n images of sh x sw on a device of num_cu compute units (0: 256); pin_seg != 0 fixes rw_seg.  Fills everything
// but the pointers, src_u8, zero / zero_n, num_cu and desc_list_cap, which belong to the call.  OP_OK, or the error set and
// OP_ERR_UNSUPPORTED (octave / scale count, Gaussian kernel over 31 taps) / OP_ERR_INVALID (an image or octave too small).
int build_plan(const op_config& cfg, int n, int sh, int sw, SiftPlan& p, int num_cu = 256, int pin_seg = 0);
