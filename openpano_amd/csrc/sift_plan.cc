// sift_plan.cc -- the plan of a SIFT batch (sift_plan.hpp): pure arithmetic on an op_config and three integers, plain C++.
// run_group (sift_host.hip) is its one caller in the library; tests/harness/sift_plan_harness.cc runs it under the sanitizers.
#include "sift_plan.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

// feature/gaussian.cc:17-40 (GaussCache) + gaussian.hh:96-103 (sigma bank), host side
static int build_gauss_bank(const op_config& cfg, SiftPlan& p) {
	float sigma = cfg.GAUSS_SIGMA;
	p.halo = 0;
	memset(p.kern, 0, sizeof(p.kern));
	memset(p.kcenter, 0, sizeof(p.kcenter));
	for (int s = 1; s < cfg.NUM_SCALE; ++s) {
		int kw = (int)(std::ceil(0.3 * (sigma / 2 - 1) + 0.8) * cfg.GAUSS_WINDOW_FACTOR);
		if (kw % 2 == 0) kw++;
		const int center = kw / 2;
		if (center > OP_MAX_KCENTER || kw < 1) return -1;
		float* kernel = &p.kern[s][OP_MAX_KCENTER];
		kernel[0] = 1;
		float exp_coeff = (float)(-1.0 / (sigma * sigma * 2)), wsum = 1;
		for (int i = 1; i <= center; i++)
			wsum += (kernel[i] = std::exp((float)(i * i) * exp_coeff)) * 2;   // std::exp(float) = expf
		float fac = (float)(1.0 / wsum);
		kernel[0] = fac;
		for (int i = 1; i <= center; i++)
			kernel[-i] = (kernel[i] *= fac);
		p.kcenter[s] = center;
		p.halo = std::max(p.halo, center);
		sigma *= cfg.SCALE_FACTOR;
	}
	return 0;
}

int build_plan(const op_config& cfg, int n, int sh, int sw, SiftPlan& p, int num_cu, int pin_seg) {
	memset(&p, 0, sizeof(p));
	if (cfg.NUM_OCTAVE < 1 || cfg.NUM_OCTAVE > OP_MAX_OCT || cfg.NUM_SCALE < 4 || cfg.NUM_SCALE > OP_MAX_SCALE)
		OP_FAIL(OP_ERR_UNSUPPORTED, "NUM_OCTAVE must be in [1,8] and NUM_SCALE in [4,12]");
	if (sh < 2 || sw < 2) OP_FAIL(OP_ERR_INVALID, "image must be at least 2x2 (lib/imgproc.cc:321)");
	p.n = n; p.sh = sh; p.sw = sw;
	// feature/feature.cc:33-34
	float ratio = cfg.SIFT_WORKING_SIZE * 2.0f / (sw + sh);
	p.wh = (int)(sh * ratio); p.ww = (int)(sw * ratio);
	if (p.wh < 2 || p.ww < 2) OP_FAIL(OP_ERR_INVALID, "working image degenerate");
	p.noct = cfg.NUM_OCTAVE; p.nscale = cfg.NUM_SCALE;
	long long off = 0; int tile_begin = 0;
	for (int i = 0; i < p.noct; ++i) {
		OctDesc& o = p.oct[i];
		if (i == 0) { o.h = p.wh; o.w = p.ww; }
		else {      // feature/dog.cc:105-107
			float factor = (float)std::pow((double)cfg.SCALE_FACTOR, (double)-i);
			o.w = (int)std::ceil(p.ww * factor); o.h = (int)std::ceil(p.wh * factor);
			if (!(o.w > 5 && o.h > 5)) OP_FAIL(OP_ERR_INVALID, "octave smaller than 6 px (feature/dog.cc:108 assertion)");
		}
		o.plane = (long long)o.h * o.w;
		o.off = off; off += o.plane * planes_per_octave(p.nscale);
		o.tiles_x = (o.w + OP_PYR_TW - 1) / OP_PYR_TW; o.tiles_y = (o.h + OP_PYR_TH - 1) / OP_PYR_TH;
		o.tile_begin = tile_begin; tile_begin += o.tiles_x * o.tiles_y;
	}
	p.total_tiles = tile_begin;
	p.ws_stride = (off + 63) & ~63LL;
	if (build_gauss_bank(cfg, p) != 0) OP_FAIL(OP_ERR_UNSUPPORTED, "Gaussian kernel wider than 31 taps");
	{
		static const int shipped[6] = {3, 3, 3, 6, 6, 6};
		p.rows_ok = p.nscale == 7;
		for (int s = 1; s < 7 && p.rows_ok; ++s) if (p.kcenter[s] != shipped[s - 1]) p.rows_ok = 0;
		if (p.rows_ok) {
			// work items of k_pyramid_rows: bands of OP_RW_OWN columns x segments of rw_seg rows.
			// Every segment re-reads 14 halo rows and adds three rows of redundant passes; long segments pay in ramp-up
			// and tail (a workgroup's lifetime grows with the segment).  On a large batch the height hardly matters
			// (config 4, 38 images = 8 fills of the device: 20 / 24 / 28 / 40 / 48 rows = 0.376 / 0.374 / 0.373 / 0.371 / 0.376 ms,
			// profiles/r06_sift_seg.txt).  On a small one it decides how many times the device is filled: four workgroups
			// fit a CU (LDS), and 5 images at 24 rows are 1065 workgroups on 1024 places -- 41 of them run alone behind the
			// rest and the kernel takes two workgroup lifetimes instead of one.  So the height is chosen per batch: the one
			// that minimises (fills of the device, rounded up) x (a workgroup's steps at that height).
			auto items_at = [&](int seg) {
				long long it = 0;
				for (int i = 0; i < p.noct; ++i) it += (long long)((p.oct[i].w + OP_RW_OWN - 1) / OP_RW_OWN) * ((p.oct[i].h + seg - 1) / seg);
				return it;
			};
			int seg = OP_RW_SEG_DEFAULT;
			if (pin_seg) seg = pin_seg;
			else {
				const long long places = (long long)(num_cu > 0 ? num_cu : 256) * 4;
				auto cost_at = [&](int c) {
					const long long items = items_at(c) * n;
					const long long fills = (items + places - 1) / places;
					return (double)fills * ((c + 3) / 2 + 1.2);       // steps of a workgroup: row pairs + the 14-row window fill (~1.2 steps)
				};
				const double dflt = cost_at(OP_RW_SEG_DEFAULT);
				double best = dflt;
				for (int c = OP_RW_SEG_MIN; c <= OP_RW_SEG_MAX; c += 2) {
					const double cost = cost_at(c);
					if (cost < best) { best = cost; seg = c; }
				}
				if (best > 0.93 * dflt) seg = OP_RW_SEG_DEFAULT;       // the model is coarse: only a clear win moves the height (measured: equal within 1 % on 8 fills)
			}
			p.rw_seg = seg;
			p.rw_items = 0;
			for (int i = 0; i < p.noct; ++i) {
				OctDesc& o = p.oct[i];
				o.rw_nb = (o.w + OP_RW_OWN - 1) / OP_RW_OWN;
				o.rw_nseg = (o.h + seg - 1) / seg;
				p.rw_items += o.rw_nb * o.rw_nseg;
			}
		}
		if (p.rows_ok)
			for (int pl = 0; pl < 3; ++pl) for (int d = 0; d < 7; ++d) for (int e = 0; e < 2; ++e) {
				const int s = 2 * pl + 1 + e;
				p.kpair[pl][d][e] = d <= p.kcenter[s] ? p.kern[s][OP_MAX_KCENTER + d] : 0.f;
			}
	}
	p.pre_color_thres = cfg.PRE_COLOR_THRES; p.judge_thres = cfg.JUDGE_EXTREMA_DIFF_THRES;
	p.contrast_thres = cfg.CONTRAST_THRES; p.edge_ratio = cfg.EDGE_RATIO; p.offset_thres = cfg.OFFSET_THRES;
	p.calc_offset_depth = cfg.CALC_OFFSET_DEPTH;
	p.gauss_sigma = cfg.GAUSS_SIGMA; p.scale_factor = cfg.SCALE_FACTOR; p.ori_radius = cfg.ORI_RADIUS;
	p.ori_smooth = cfg.ORI_HIST_SMOOTH_COUNT; p.desc_scale_factor = cfg.DESC_HIST_SCALE_FACTOR;
	p.desc_int_factor = cfg.DESC_INT_FACTOR;
	return OP_OK;
}
