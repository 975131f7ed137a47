// sift_plan_harness.cc -- the plan of a SIFT batch (csrc/sift_plan.cc) as a program of its own, for the sanitizers: build_plan
// indexes the Gaussian bank and the octave table by hand from caller-supplied NUM_SCALE, NUM_OCTAVE and GAUSS_WINDOW_FACTOR.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I csrc
//       sift_plan_harness.cc csrc/sift_plan.cc
// Reads one case per line from the file named on the command line:
//   SIFT_WORKING_SIZE NUM_OCTAVE NUM_SCALE SCALE_FACTOR GAUSS_SIGMA GAUSS_WINDOW_FACTOR n sh sw num_cu pin_seg
// (the two floats as the hex of their bit patterns) and prints each plan as one line of JSON, floats again as bit patterns;
// tests/test_sift_plan_cpu.py checks the numbers.
#include "sift_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static std::string g_error;
void op_set_error(const std::string& msg) { g_error = msg; }

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float from_bits(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); exit(1); } } while (0)

int main(int argc, char** argv) {
	FILE* in = argc > 1 ? fopen(argv[1], "r") : nullptr;
	EXPECT(in);
	char line[512];
	int cases = 0;
	while (fgets(line, sizeof line, in)) {
		op_config c;
		memset(&c, 0, sizeof c);
		unsigned sf, sigma;
		int n, sh, sw, num_cu, pin;
		EXPECT(sscanf(line, "%d %d %d %x %x %d %d %d %d %d %d", &c.SIFT_WORKING_SIZE, &c.NUM_OCTAVE, &c.NUM_SCALE, &sf, &sigma,
				&c.GAUSS_WINDOW_FACTOR, &n, &sh, &sw, &num_cu, &pin) == 11);
		c.SCALE_FACTOR = from_bits(sf); c.GAUSS_SIGMA = from_bits(sigma);
		c.CONTRAST_THRES = 4e-2f; c.EDGE_RATIO = 6.f; c.CALC_OFFSET_DEPTH = 4; c.ORI_RADIUS = 4.5f; c.DESC_INT_FACTOR = 512;
		SiftPlan* p = new SiftPlan;           // on the heap: a write past the struct is the sanitizer's to see
		g_error.clear();
		const int rc = build_plan(c, n, sh, sw, *p, num_cu, pin);
		printf("{\"rc\": %d, \"error\": \"%s\"", rc, g_error.c_str());
		if (rc == OP_OK) {
			// what the plan copies from the config and what it leaves to the call
			EXPECT(p->n == n && p->sh == sh && p->sw == sw && p->noct == c.NUM_OCTAVE && p->nscale == c.NUM_SCALE);
			EXPECT(p->contrast_thres == c.CONTRAST_THRES && p->edge_ratio == c.EDGE_RATIO && p->calc_offset_depth == c.CALC_OFFSET_DEPTH);
			EXPECT(p->ori_radius == c.ORI_RADIUS && p->desc_int_factor == c.DESC_INT_FACTOR && p->gauss_sigma == c.GAUSS_SIGMA && p->scale_factor == c.SCALE_FACTOR);
			EXPECT(!p->ws && !p->work && !p->srcs && !p->zero && !p->zero_n && !p->num_cu && !p->desc_list_cap && !p->src_u8);
			printf(", \"wh\": %d, \"ww\": %d, \"halo\": %d, \"total_tiles\": %d, \"ws_stride\": %lld, \"rows_ok\": %d, \"rw_seg\": %d, \"rw_items\": %d",
					p->wh, p->ww, p->halo, p->total_tiles, p->ws_stride, p->rows_ok, p->rw_seg, p->rw_items);
			printf(", \"oct\": [");
			for (int i = 0; i < p->noct; ++i) {
				const OctDesc& o = p->oct[i];
				printf("%s[%d, %d, %d, %d, %d, %d, %d, %lld, %lld]", i ? ", " : "", o.h, o.w, o.tiles_x, o.tiles_y, o.tile_begin, o.rw_nb, o.rw_nseg, o.off, o.plane);
			}
			printf("], \"kcenter\": [");
			for (int s = 0; s < OP_MAX_SCALE; ++s) printf("%s%d", s ? ", " : "", p->kcenter[s]);
			printf("], \"kern\": [");
			for (int s = 0; s < OP_MAX_SCALE; ++s)
				for (int k = 0; k < 2 * OP_MAX_KCENTER + 1; ++k) printf("%s%u", s + k ? ", " : "", bits(p->kern[s][k]));
			printf("], \"kpair\": [");
			for (int pl = 0; pl < 3; ++pl) for (int d = 0; d < 7; ++d) for (int e = 0; e < 2; ++e) printf("%s%u", pl + d + e ? ", " : "", bits(p->kpair[pl][d][e]));
			printf("]");
		}
		printf("}\n");
		delete p;
		++cases;
	}
	fclose(in);
	printf("sift_plan_harness: %d plans\n", cases);
	return 0;
}
