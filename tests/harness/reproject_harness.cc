// reproject_harness.cc -- the host side of the re-projection (csrc/pano_angle.hpp, and op_pano_frame_of, op_view_look,
// op_view_cube_face, op_view_planet and op_canvas_reproject's refusals in csrc/blend_geom.cc) as a program of its own, for the
// sanitizers; and the maps themselves on one host thread (reproject_host, the C++ twin of tests/reproject_cases.py), which
// tests/test_reproject_cpu.py holds to the numpy restatement and scripts/reproject_probe.py times.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I include -I csrc
//       reproject_harness.cc csrc/blend_geom.cc
//   reproject_harness atan2 IN OUT          IN: pairs (y, x) of doubles; OUT: pano_atan2 of each
//   reproject_harness helpers FILE          one call per line of FILE (numbers as C99 hex floats); prints "rc values..." per line:
//       frame METHOD MINX MINY RESX RESY X0 Y0 | look YAW PITCH ROLL HFOV W H | cube FACE N | planet N
//       check LON0 LAT0 STEP_LON STEP_LAT WRAP MODE OUT_H OUT_W FOCAL ROT0..ROT8
//   reproject_harness render SRC H W OUT LON0 LAT0 STEP_LON STEP_LAT WRAP MODE OUT_H OUT_W FOCAL ROT0..ROT8
//                                           SRC: H x W x 3 floats; OUT: OUT_H x OUT_W x 3 floats
//   reproject_harness --time WHAT H W N     WHAT: planet (1000 x 1000), view (1920 x 1080) or cube (six 1024 x 1024) from a synthetic
//                                           H x W canvas, N times; prints the milliseconds of the fastest
#include "blend_shared.hpp"
#include "pano_angle.hpp"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

static std::string g_error;
void op_set_error(const std::string& msg) { g_error = msg; }

static void die(const char* what) { fprintf(stderr, "reproject_harness: %s\n", what); exit(2); }

// interpolate (lib/imgproc.cc:135-156); false = Color::NO.  wrap: csrc/reproject.hip's interpolate_wrap
static bool sample(const float* img, int rows, int cols, float r, float c, bool wrap, float (&out)[3]) {
	if (wrap ? !(r >= 0.f && c >= 0.f && r < (float)(rows - 1) && c <= (float)cols) : !(r >= 0.f && c >= 0.f && r < (float)(rows - 1) && c < (float)(cols - 1)))
		return false;
	const int fr = (int)std::floor(r);
	int fc = (int)std::floor(c);
	r -= (float)fr; c -= (float)fc;
	if (fc >= cols) { fc = 0; c = 0.f; }
	const int fc1 = fc + 1 == cols ? 0 : fc + 1;
	const float* row0 = img + (size_t)fr * cols * 3;
	const float* row1 = row0 + (size_t)cols * 3;
	const float* p[4] = {row0 + fc * 3, row1 + fc * 3, row1 + fc1 * 3, row0 + fc1 * 3};
	if (p[0][0] < 0 || p[1][0] < 0 || p[2][0] < 0 || p[3][0] < 0) return false;
	const float w[4] = {(1 - r) * (1 - c), r * (1 - c), r * c, (1 - r) * c};
	for (int ch = 0; ch < 3; ++ch) {
		float s = 0.f;
		for (int q = 0; q < 4; ++q) s += p[q][ch] * w[q];
		out[ch] = s;
	}
	return true;
}

// k_canvas_reproject on one host thread
static void reproject_host(const float* src, int H, int W, const op_pano_frame& F, const op_view_spec& S, float* out) {
	const bool wrap = F.wrap != 0;
	for (int i = 0; i < S.out_h; ++i)
		for (int j = 0; j < S.out_w; ++j) {
			float col[3];
			bool ok = false;
			if (H < 1 || W < 1) {
			} else if (S.mode == OP_VIEW_PLANET) {
				const int center = S.out_w / 2;
				const int di = center - i, dj = center - j;
				double dist = std::sqrt((double)((long long)di * di + (long long)dj * dj));
				if (!(dist >= (double)center || dist == 0)) {
					dist = dist / (double)center;
					dist = (double)H - dist * (double)H;
					double theta;
					if (j == center) theta = i < center ? PANO_PI / 2 : 3 * PANO_PI / 2;
					else {
						theta = pano_atan2((double)di / (double)dj, 1.0);
						if (theta < 0) theta += PANO_PI;
						if (theta == 0 && j > center) theta += PANO_PI;
						if (center < i) theta += PANO_PI;
					}
					theta = theta / (PANO_PI * 2) * (double)W;
					if ((double)(H - 1) < dist) dist = (double)(H - 1);
					ok = sample(src, H, W, (float)dist, (float)theta, wrap, col);
				}
			} else {
				const double u = (double)j - 0.5 * (double)(S.out_w - 1), v = (double)i - 0.5 * (double)(S.out_h - 1);
				const double* R = S.rot;
				const double dx = R[0] * u + R[1] * v + R[2] * S.focal;
				const double dy = R[3] * u + R[4] * v + R[5] * S.focal;
				const double dz = R[6] * u + R[7] * v + R[8] * S.focal;
				const double lon = pano_atan2(dx, dz);
				const double lat = pano_atan2(dy, std::sqrt(dx * dx + dz * dz));
				const double py = (lat - F.lat0) / F.step_lat;
				if (wrap) {
					double d = lon - F.lon0;
					if (d < 0) d = d + PANO_2PI;
					if (d >= PANO_2PI) d = d - PANO_2PI;
					const double px = d / (PANO_PI * 2) * (double)W;
					if (!(py < 0 || py >= H) && !(px != px)) ok = sample(src, H, W, (float)py, (float)px, true, col);
				} else {
					const double px = (lon - F.lon0) / F.step_lon;
					if (!(px < 0 || px >= W || py < 0 || py >= H) && !(px != px)) ok = sample(src, H, W, (float)py, (float)px, false, col);
				}
			}
			float* p = out + ((size_t)i * S.out_w + j) * 3;
			for (int ch = 0; ch < 3; ++ch) p[ch] = ok ? col[ch] : -1.f;
		}
}

static std::vector<char> read_file(const char* path) {
	FILE* f = fopen(path, "rb");
	if (!f) die("cannot open the input");
	std::vector<char> buf;
	char chunk[65536];
	size_t n;
	while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
	fclose(f);
	return buf;
}
static void write_file(const char* path, const void* data, size_t bytes) {
	FILE* f = fopen(path, "wb");
	if (!f || fwrite(data, 1, bytes, f) != bytes) die("cannot write the output");
	fclose(f);
}
static double num(const std::string& s) {
	char* end = nullptr;
	const double v = strtod(s.c_str(), &end);
	if (end == s.c_str() || *end) die("not a number");
	return v;
}
// LON0 LAT0 STEP_LON STEP_LAT WRAP MODE OUT_H OUT_W FOCAL ROT0..ROT8 from w[at...]
static void frame_and_spec(const std::vector<std::string>& w, size_t at, op_pano_frame& F, op_view_spec& S) {
	if (w.size() < at + 18) die("too few numbers");
	F.lon0 = num(w[at]); F.lat0 = num(w[at + 1]); F.step_lon = num(w[at + 2]); F.step_lat = num(w[at + 3]); F.wrap = (int)num(w[at + 4]);
	S.mode = (int)num(w[at + 5]); S.out_h = (int)num(w[at + 6]); S.out_w = (int)num(w[at + 7]); S.focal = num(w[at + 8]);
	for (int k = 0; k < 9; ++k) S.rot[k] = num(w[at + 9 + k]);
}
static void print_spec(int rc, const op_view_spec& S) {
	printf("%d %d %d %d %a", rc, S.mode, S.out_h, S.out_w, S.focal);
	for (int k = 0; k < 9; ++k) printf(" %a", S.rot[k]);
	printf("\n");
}

static int helpers(const char* path) {
	const std::vector<char> buf = read_file(path);
	std::istringstream in(std::string(buf.begin(), buf.end()));
	std::string line;
	while (std::getline(in, line)) {
		std::istringstream ls(line);
		std::vector<std::string> w;
		for (std::string t; ls >> t;) w.push_back(t);
		if (w.empty()) continue;
		op_view_spec S;
		memset(&S, 0, sizeof(S));
		if (w[0] == "frame" && w.size() == 8) {
			op_blend_geom g;
			memset(&g, 0, sizeof(g));
			g.proj_method = (int)num(w[1]); g.proj_min[0] = num(w[2]); g.proj_min[1] = num(w[3]); g.resolution[0] = num(w[4]); g.resolution[1] = num(w[5]);
			op_pano_frame F;
			memset(&F, 0, sizeof(F));
			F.wrap = 7;
			const int rc = op_pano_frame_of(&g, (int)num(w[6]), (int)num(w[7]), &F);
			printf("%d %a %a %a %a %d\n", rc, F.lon0, F.lat0, F.step_lon, F.step_lat, F.wrap);
		} else if (w[0] == "look" && w.size() == 7) {
			const int rc = op_view_look(num(w[1]), num(w[2]), num(w[3]), num(w[4]), (int)num(w[5]), (int)num(w[6]), &S);
			print_spec(rc, S);
		} else if (w[0] == "cube" && w.size() == 3) {
			const int rc = op_view_cube_face((int)num(w[1]), (int)num(w[2]), &S);
			print_spec(rc, S);
		} else if (w[0] == "planet" && w.size() == 2) {
			const int rc = op_view_planet((int)num(w[1]), &S);
			print_spec(rc, S);
		} else if (w[0] == "check") {
			op_pano_frame F;
			frame_and_spec(w, 1, F, S);
			g_error.clear();
			const int rc = reproject_check(&F, &S);
			printf("%d %s\n", rc, g_error.c_str());
		} else die("unknown helper line");
	}
	// NULL arguments are refused by every helper
	op_view_spec S; op_pano_frame F; op_blend_geom g;
	memset(&g, 0, sizeof(g)); g.proj_method = 2;
	const int nulls[] = {op_pano_frame_of(nullptr, 0, 0, &F), op_pano_frame_of(&g, 0, 0, nullptr), op_view_look(0, 0, 0, 1, 4, 4, nullptr),
		op_view_cube_face(0, 4, nullptr), op_view_planet(4, nullptr), reproject_check(nullptr, &S), reproject_check(&F, nullptr)};
	for (int rc : nulls) if (rc != OP_ERR_INVALID) die("a NULL argument was not refused");
	printf("reproject_harness: helpers done\n");
	return 0;
}

int main(int argc, char** argv) {
	if (argc == 4 && !strcmp(argv[1], "atan2")) {
		const std::vector<char> buf = read_file(argv[2]);
		const size_t n = buf.size() / (2 * sizeof(double));
		std::vector<double> in(2 * n), out(n);
		if (n) memcpy(in.data(), buf.data(), 2 * n * sizeof(double));
		for (size_t k = 0; k < n; ++k) out[k] = pano_atan2(in[2 * k], in[2 * k + 1]);
		write_file(argv[3], out.data(), n * sizeof(double));
		printf("reproject_harness: %zu angles\n", n);
		return 0;
	}
	if (argc == 3 && !strcmp(argv[1], "helpers")) return helpers(argv[2]);
	if (argc == 24 && !strcmp(argv[1], "render")) {
		const int H = atoi(argv[3]), W = atoi(argv[4]);
		const std::vector<char> buf = read_file(argv[2]);
		if (H < 0 || W < 0 || buf.size() != (size_t)H * W * 3 * sizeof(float)) die("the source has another size");
		std::vector<float> src((size_t)H * W * 3 + 1);
		if (!buf.empty()) memcpy(src.data(), buf.data(), buf.size());
		std::vector<std::string> w(argv + 6, argv + argc);
		op_pano_frame F; op_view_spec S;
		frame_and_spec(w, 0, F, S);
		if (reproject_check(&F, &S) != OP_OK) die(g_error.c_str());
		std::vector<float> out((size_t)S.out_h * S.out_w * 3);
		reproject_host(src.data(), H, W, F, S, out.data());
		write_file(argv[5], out.data(), out.size() * sizeof(float));
		return 0;
	}
	if (argc == 6 && !strcmp(argv[1], "--time")) {
		const std::string what = argv[2];
		const int H = atoi(argv[3]), W = atoi(argv[4]), N = atoi(argv[5]);
		if (H < 1 || W < 1 || N < 1) die("--time WHAT H W N");
		std::vector<float> src((size_t)H * W * 3);
		unsigned s = 12345;
		for (float& v : src) { s = s * 1664525u + 1013904223u; v = (float)(s >> 8) * (1.f / 16777216.f); }
		op_pano_frame F = {-PANO_PI, -PANO_PI_2 * 0.2, PANO_2PI / W, PANO_PI * 0.2 / H, 1};
		std::vector<op_view_spec> specs;
		op_view_spec S;
		if (what == "planet") { if (op_view_planet(1000, &S) != OP_OK) die("planet"); specs.push_back(S); }
		else if (what == "view") { if (op_view_look(0.3, 0.02, 0.0, 1.2, 1920, 1080, &S) != OP_OK) die("view"); specs.push_back(S); }
		else if (what == "cube") for (int f = 0; f < 6; ++f) { if (op_view_cube_face(f, 1024, &S) != OP_OK) die("cube"); specs.push_back(S); }
		else die("--time: planet, view or cube");
		std::vector<float> out((size_t)specs[0].out_h * specs[0].out_w * 3);
		double best = 1e300, sink = 0;
		for (int k = 0; k < N; ++k) {
			const auto t0 = std::chrono::steady_clock::now();
			for (const op_view_spec& sp : specs) { reproject_host(src.data(), H, W, F, sp, out.data()); sink += out[out.size() / 2]; }
			best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
		}
		printf("%.3f ms (%g)\n", best, sink);
		return 0;
	}
	die("usage: atan2 IN OUT | helpers FILE | render SRC H W OUT <18 numbers> | --time WHAT H W N");
	return 2;
}
