// stitch_demo.cc -- standalone C++ host program over the adapters of pano_hip.hh (no reference
// tree, no Python): the hot path in the order Stitcher::build() runs it (stitch/stitcher.cc:32-64),
//   calc_feature -> pairwise_match (+ RANSAC per pair) -> [host camera estimation: out of scope,
//   replaced here by chaining the pairwise homographies to the middle image] -> blend,
// written with the reference's class and method names.
//
//   stitch_demo <in.bin> <out.bin> [base_seed] [camera|camera_ordered|camera_build|cylinder|cylinder_build|reproject]
// ("camera_ordered": ORDERED_INPUT 1 as in BASELINE configs 2-3 -- only (i, i+1 mod n) are matched,
// Stitcher::linear_pairwise_match, stitcher.cc:115-136; head and tail need not connect.)
// With "camera" the program runs the ESTIMATE_CAMERA branch of Stitcher::build() instead (BASELINE
// configs 2-4): all pairs matched, homography RANSAC, host camera estimation + bundle adjustment
// (pano_camera.hh), spherical blend; out.bin then carries n*13 f64 cameras (focal, aspect, ppx,
// ppy, R) in place of the chain homographies, before the canvas.
// "camera_build": the same branch through HipStitcher::build() itself (Stitcher st(mats); st.build()); out.bin then
// holds only int32 H, W ; H*W*3 f32 [; n*3 f32 gains under --gain-compensation, n*B*3 under --gain-blocks].
// "cylinder": CylinderStitcher::build() (stitch/cylstitcher.cc:20-29; CYLINDER 1, ESTIMATE_CAMERA 0, TRANS 0, ORDERED_INPUT 1,
// LAZY_READ 0) stage by stage through HipCylinderStitcher, from in.bin or --jpeg-list [--jpeg-orient]; accepts --resident-views,
// --png, --jpeg.. and --crop, and encodes the files from the device canvas.  out.bin then holds
//          int32 n ; per view int32 K ; K*2 f64 keypoints as detected
//          int32 number of update_h_factor attempts ; per attempt f32 factor, f32 slope, int32 ok ; f32 best factor
//          n*9 f64 component.homo ; int32 H, W ; H*W*3 f32 (the blend, before the correction)
//          8 f64 corners ; 9 f64 inv ; int32 H, W ; H*W*3 f32 (the panorama)
// "cylinder_build": the same through HipCylinderStitcher::build() itself, then hip_perspective_correction(bundle, Mat32f) on the
// blend of that build, then build_canvas(crop) on the same object, from which the files are encoded; out.bin then holds three
// times int32 H, W ; H*W*3 f32: the first two the panorama, the third the panorama cropped under --crop.  --profile (this mode
// only) prints the context's stage times and the wall time of that build_canvas() call to stderr.
// --crop (anywhere; cylinder modes only): the files of --png / --jpeg hold the panorama cropped to its largest valid rectangle
// (crop(), lib/imgproc.cc:200-235, on the device); out.bin is the same with and without it.
// --gain-compensation (anywhere on the line): exposure compensation before the blend (HipStitcher::gain_compensation,
// hip_gain_compensate: an extension beyond the reference); out.bin then ends with n*3 f32 gains after the canvas.
// --gain-blocks BXxBY (anywhere; implies --gain-compensation): block gain compensation on a BX x BY grid per image
// (HipStitcher::gain_blocks_x / _y, hip_gain_compensate_blocks; 1x1 is --gain-compensation itself); out.bin then ends
// with n*BY*BX*3 f32 gains, [((k*BY + v)*BX + u)*3 + c], after the canvas (camera modes) or the chain homographies.
// --vignetting (anywhere; not with --gain-blocks): grey gains plus one radial falloff curve shared by all views
// (HipStitcher::vignetting, hip_vignette_compensate); out.bin then ends with n*3 f32 gains and the curve's 3 f32
// coefficients a1, a2, a3, where --gain-compensation puts its gains.
// --png PATH (anywhere): additionally writes the panorama out.bin holds as an 8-bit RGB PNG, encoded on the device
// (hip_write_png: write_rgb's quantisation, lib/imgio.cc:25-41); out.bin is the same with and without it.
// --jpeg PATH [--jpeg-quality Q] [--jpeg-444] (anywhere): additionally writes the panorama out.bin holds as a baseline JPEG,
// encoded on the device (hip_write_jpeg: write_rgb's quantisation, lib/imgio.cc:98-113); quality 90 and 4:2:0 unless told
// otherwise; out.bin is the same with and without it.
// --resident-views (anywhere): the images are uploaded once (HipStitcher::resident_views; bytes when every pixel is an exact
// k / 255, fp32 otherwise) and SIFT, the overlap passes and the blend read that upload; out.bin is the same with and without it.
// --jpeg-list PATH (anywhere; camera modes only): PATH is a text file with one baseline JPEG path per line.  The files stand in
// place of in.bin's contents (in.bin is not opened) and are decoded on the device (HipStitcher over jpeg_paths,
// hip_read_jpeg_views); implies --resident-views.  out.bin equals a run on an in.bin that holds the same decoded pixels.
// --jpeg-orient (anywhere; with --jpeg-list only): every view is turned upright by its file's EXIF orientation, which the
// reference's decoder ignores (HipStitcher::apply_exif_orientation).  out.bin equals a run on an in.bin that holds the decoded
// pixels turned beforehand.
// "reproject": in.bin is a finished equirectangular panorama as this program writes one (int32 H, W ; H*W*3 f32, Color::NO = -1
// allowed); it goes up once and is looked at again on the device (hip_reproject), as ONE of
//   --planet N                          the reference's planet (main.cc:294-331) of N x N pixels
//   --view YAW,PITCH,ROLL,HFOV,WxH      a pinhole view, angles in radians (hip_view_look)
//   --cube N                            the six faces +x, -x, +y, -y, +z, -z of N x N pixels (hip_view_cube_face)
// --frame LON0,LAT0,STEP_LON,STEP_LAT says where the panorama sits on the sphere (op_pano_frame; numbers as strtod reads them, hex
// floats included); without it: square pixels of 2 pi / W, column 0 at -pi, the middle row on the horizon.  --wrap states that the
// columns span exactly one turn.  out.bin then holds int32 H, W ; H*W*3 f32 per view (six for --cube), and --png / --jpeg name the
// encoded view; for --cube six files, the face's suffix (_px _nx _py _ny _pz _nz) in front of the extension.
// The same three options (and --wrap) go with camera_build: the panorama stays on the device (HipStitcher::build_canvas), its frame
// comes from the bundle (HipStitcher::pano_frame), out.bin ends with the views, and --png / --jpeg name the views, not the panorama.
// in.bin : int32 n, h, w ; n*h*w*3 float32 (Mat32f layout)
// out.bin: per image   int32 K ; K*128 f32 ; K*2 f64
//          int32 npairs ; per pair int32 i, j, M ; M*2 int32 ; int32 ok ; f32 confidence ; 9 f64 ; int32 ninl ; ninl*4 f64
//          int32 H, W ; H*W*3 f32 (flat-projection linear blend of the chain that connected; H=W=0 if none)
// tests/test_gpu_host_cpp.py runs it on the GPU box and checks every section against the oracle.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pano_hip.hh"

using namespace pano;

// what the command line asks for
struct Options {
	const char* out_path = nullptr;
	uint32_t base_seed = 42u;
	std::string mode;
	HipCompensation compensation;       // --gain-compensation, --gain-blocks BXxBY, --vignetting
	const char* png_path = nullptr;     // --png PATH
	const char* jpeg_path = nullptr;    // --jpeg PATH, --jpeg-quality Q, --jpeg-444
	int jpeg_quality = 90;
	bool jpeg_444 = false;
	bool resident = false;              // --resident-views
	const char* jpeg_list = nullptr;    // --jpeg-list PATH, --jpeg-orient
	bool jpeg_orient = false;
	bool crop = false, profile = false; // --crop, --profile
	// what to make of the finished panorama: --planet N, --view Y,P,R,HFOV,WxH, --cube N; --wrap, --frame
	enum View { NO_VIEW, PLANET, LOOK, CUBE } view = NO_VIEW;
	int view_n = 0, view_w = 0, view_h = 0;
	double look[4] = {0, 0, 0, 0};
	bool wrap = false, has_frame = false;
	double frame[4] = {0, 0, 0, 0};
};

template <typename T> static void put(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { perror("write"); exit(1); } }
template <typename T> static void put1(FILE* f, T v) { put(f, &v, 1); }
// int32 H, W ; H*W*3 f32, from host memory or from a device canvas
static void put_mat(FILE* fo, const Mat32f& m) {
	put1<int32_t>(fo, m.rows()); put1<int32_t>(fo, m.cols());
	put(fo, m.ptr(), (size_t)m.rows() * m.cols() * 3);
}
static void put_canvas(FILE* fo, const op_canvas* cv) {
	int h, w;
	PANO_HIP_CHECK(op_canvas_dims(cv, &h, &w));
	std::vector<float> px((size_t)h * w * 3);
	if (!px.empty()) PANO_HIP_CHECK(op_canvas_copy(HipContext::get(), cv, px.data()));
	put1<int32_t>(fo, h); put1<int32_t>(fo, w);
	put(fo, px.data(), px.size());
}
// the files of --png / --jpeg, encoded on the device from a host matrix or from a device canvas
template <typename Pano> static void write_files(const Options& o, const Pano& pano) {
	if (o.png_path) hip_write_png(o.png_path, pano);
	if (o.jpeg_path) hip_write_jpeg(o.jpeg_path, pano, o.jpeg_quality, o.jpeg_444 ? OP_JPEG_444 : OP_JPEG_420);
}

// "out.png" + "_px" -> "out_px.png"
static std::string with_suffix(const char* path, const char* suffix) {
	const std::string p(path);
	const size_t dot = p.rfind('.'), slash = p.rfind('/');
	if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return p + suffix;
	return p.substr(0, dot) + suffix + p.substr(dot);
}
// the view(s) the options ask for, of the device panorama lying at `frame`: appended to out.bin, encoded into the files
static void put_views(FILE* fo, const Options& o, const op_canvas* pano, const op_pano_frame& frame) {
	static const char* const FACE[6] = {"_px", "_nx", "_py", "_ny", "_pz", "_nz"};
	const int count = o.view == Options::CUBE ? 6 : 1;
	fprintf(stderr, "Frame: %a %a %a %a %d\n", frame.lon0, frame.lat0, frame.step_lon, frame.step_lat, frame.wrap);
	for (int k = 0; k < count; ++k) {
		const op_view_spec spec = o.view == Options::PLANET ? hip_view_planet(o.view_n)
			: o.view == Options::CUBE ? hip_view_cube_face(k, o.view_n)
			: hip_view_look(o.look[0], o.look[1], o.look[2], o.look[3], o.view_w, o.view_h);
		HipCanvas view(hip_reproject(pano, frame, spec));
		put_canvas(fo, view.get());
		const char* suffix = o.view == Options::CUBE ? FACE[k] : "";
		if (o.png_path) hip_write_png(with_suffix(o.png_path, suffix).c_str(), view.get());
		if (o.jpeg_path) hip_write_jpeg(with_suffix(o.jpeg_path, suffix).c_str(), view.get(), o.jpeg_quality, o.jpeg_444 ? OP_JPEG_444 : OP_JPEG_420);
		fprintf(stderr, "View %d Size: (%d, %d)\n", k, spec.out_w, spec.out_h);
	}
}

// a finished panorama from in.bin, looked at again
static int run_reproject(const char* in_path, const Options& o) {
	if (o.view == Options::NO_VIEW) { fprintf(stderr, "reproject wants --planet N, --view YAW,PITCH,ROLL,HFOV,WxH or --cube N\n"); return 2; }
	FILE* fi = fopen(in_path, "rb");
	if (!fi) { perror(in_path); return 2; }
	int32_t hw[2];
	if (fread(hw, 4, 2, fi) != 2 || hw[0] < 1 || hw[1] < 1) { fprintf(stderr, "%s: no panorama (int32 H, W ; H*W*3 f32)\n", in_path); return 2; }
	Mat32f pano(hw[0], hw[1], 3);
	if (fread(pano.ptr(), sizeof(float), (size_t)hw[0] * hw[1] * 3, fi) != (size_t)hw[0] * hw[1] * 3) { fprintf(stderr, "%s: short file\n", in_path); return 2; }
	fclose(fi);
	op_pano_frame frame;
	if (o.has_frame) { frame.lon0 = o.frame[0]; frame.lat0 = o.frame[1]; frame.step_lon = o.frame[2]; frame.step_lat = o.frame[3]; }
	else {
		const double step = M_PI * 2 / hw[1];
		frame.lon0 = -M_PI; frame.step_lon = step; frame.step_lat = step; frame.lat0 = -0.5 * step * (hw[0] - 1);
	}
	frame.wrap = o.wrap ? 1 : 0;
	HipCanvas cv;
	PANO_HIP_CHECK(op_canvas_upload(HipContext::get(), pano.ptr(), pano.rows(), pano.cols(), hip_out(cv)));
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	put_views(fo, o, cv.get(), frame);
	fclose(fo);
	return 0;
}

static void put_features(FILE* fo, const HipFeatureSet& fs) {
	for (size_t k = 0; k < fs.feats.size(); ++k) {
		put1<int32_t>(fo, (int32_t)fs.feats[k].size());
		for (auto& d : fs.feats[k]) put(fo, d.descriptor.data(), 128);
		for (auto& d : fs.feats[k]) { double c[2] = {d.coor.x, d.coor.y}; put(fo, c, 2); }
		fprintf(stderr, "Image %zu has %zu features\n", k, fs.feats[k].size());
	}
}
// pwmatcher: has matched `tasks` already (precompute)
static void put_pairs(FILE* fo, const PairWiseMatcher& pwmatcher, const std::vector<std::pair<int, int>>& tasks,
		const std::vector<std::pair<bool, MatchInfo>>& infos) {
	put1<int32_t>(fo, (int32_t)tasks.size());
	for (size_t p = 0; p < tasks.size(); ++p) {
		MatchData md = pwmatcher.match(tasks[p].first, tasks[p].second);
		put1<int32_t>(fo, tasks[p].first); put1<int32_t>(fo, tasks[p].second); put1<int32_t>(fo, md.size());
		for (auto& q : md.data) { int32_t v[2] = {q.first, q.second}; put(fo, v, 2); }
		const MatchInfo& info = infos[p].second;
		put1<int32_t>(fo, infos[p].first ? 1 : 0); put1<float>(fo, info.confidence);
		double hh[9]; for (int i = 0; i < 9; ++i) hh[i] = infos[p].first ? info.homo[i] : 0.0;
		put(fo, hh, 9);
		put1<int32_t>(fo, (int32_t)(infos[p].first ? info.match.size() : 0));
		if (infos[p].first) for (auto& m : info.match) { double v[4] = {m.first.x, m.first.y, m.second.x, m.second.y}; put(fo, v, 4); }
		fprintf(stderr, "pair (%d,%d): %d matches, %s, confidence %g\n", tasks[p].first, tasks[p].second, md.size(),
				infos[p].first ? "connected" : "rejected", info.confidence);
	}
}

// Stitcher::build() under ESTIMATE_CAMERA (stitch/stitcher.cc:32-64), stage by stage so that every
// intermediate can be written out
static int run_camera_mode(Stitcher& st, const Options& o) {
	const bool ordered = o.mode == "camera_ordered";
	const HipCompensation& how = o.compensation;
	st.resident_views = o.resident;
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	st.calc_feature();
	st.bundle.views = o.resident ? st.feats.views.get() : nullptr;     // the overlap passes and the blend read the upload
	put_features(fo, st.feats);
	const int n = (int)st.imgs.size();
	st.pairwise_matches.assign(n, std::vector<MatchInfo>(n));
	const std::vector<std::pair<int, int>> tasks = hip_default_tasks(n, ordered);
	auto infos = hip_match_images(st.feats, st.shapes(), tasks, o.base_seed);
	PairWiseMatcher pwmatcher(st.feats);
	pwmatcher.precompute(tasks);
	put_pairs(fo, pwmatcher, tasks, infos);
	st.record_matches(tasks, infos, ordered);
	st.assign_center();
	st.estimate_camera();
	for (auto& c : st.cameras) {
		double v[13] = {c.focal, c.aspect, c.ppx, c.ppy};
		for (int k = 0; k < 9; ++k) v[4 + k] = c.R[k];
		put(fo, v, 13);
		fprintf(stderr, "camera focal=%g ppx=%g ppy=%g\n", c.focal, c.ppx, c.ppy);
	}
	st.bundle.proj_method = ConnectedImages::spherical;
	st.bundle.update_proj_range();
	Mat32f pano = hip_compensate_and_blend(st.bundle, how, st.gains, st.vignette_poly);
	put_mat(fo, pano);
	fprintf(stderr, "Final Image Size: (%d, %d)\n", pano.cols(), pano.rows());
	write_files(o, pano);
	if (how.gain || how.vignetting) {
		put(fo, st.gains.data(), st.gains.size());
		const size_t per = st.gains.size() / n;      // 3 per image, or 3 per block
		for (int k = 0; k < n; ++k) fprintf(stderr, "gain %d: %g %g %g\n", k, st.gains[per * k], st.gains[per * k + 1], st.gains[per * k + 2]);
	}
	if (how.vignetting) {
		put(fo, st.vignette_poly.data(), 3);
		fprintf(stderr, "vignetting curve: a = %g %g %g\n", st.vignette_poly[0], st.vignette_poly[1], st.vignette_poly[2]);
	}
	fclose(fo);
	return 0;
}

// Stitcher::build() as a client calls it, gain compensation per HipStitcher::gain_compensation
static int run_build(Stitcher& st, const Options& o) {
	st.resident_views = o.resident;
	st.gain_compensation = o.compensation.gain;
	st.vignetting = o.compensation.vignetting;
	st.gain_blocks_x = o.compensation.bx; st.gain_blocks_y = o.compensation.by;
	if (o.view != Options::NO_VIEW) {       // files -> panorama -> view: no pixel of either comes to the host but for out.bin
		HipCanvas cv(st.build_canvas());
		FILE* fo = fopen(o.out_path, "wb");
		if (!fo) { perror(o.out_path); return 2; }
		put_canvas(fo, cv.get());
		put(fo, st.gains.data(), st.gains.size());
		if (st.vignetting) put(fo, st.vignette_poly.data(), 3);
		put_views(fo, o, cv.get(), st.pano_frame(o.wrap));
		fclose(fo);
		return 0;
	}
	Mat32f pano = st.build();
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	put_mat(fo, pano);
	put(fo, st.gains.data(), st.gains.size());
	if (st.vignetting) put(fo, st.vignette_poly.data(), 3);
	fclose(fo);
	write_files(o, pano);
	fprintf(stderr, "Final Image Size: (%d, %d), %zu gains\n", pano.cols(), pano.rows(), st.gains.size());
	return 0;
}

// CylinderStitcher::build() (stitch/cylstitcher.cc:20-29), stage by stage so that every intermediate can be written out
static int run_cylinder_mode(CylinderStitcher& st, const Options& o) {
	st.resident_views = o.resident;
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	const int n = (int)st.imgs.size();
	st.calc_feature();
	put1<int32_t>(fo, n);
	for (int k = 0; k < n; ++k) {
		put1<int32_t>(fo, (int32_t)st.keypoints[k].size());
		for (auto& p : st.keypoints[k]) { double c[2] = {p.x, p.y}; put(fo, c, 2); }
		fprintf(stderr, "Image %d has %zu features\n", k, st.keypoints[k].size());
	}
	st.bundle.identity_idx = n >> 1;
	st.build_warp();
	st.free_feature();
	put1<int32_t>(fo, (int32_t)st.attempts.size());
	for (auto& a : st.attempts) { put1<float>(fo, a.factor); put1<float>(fo, a.slope); put1<int32_t>(fo, a.ok ? 1 : 0); }
	put1<float>(fo, st.best_factor);
	for (auto& c : st.bundle.component) put(fo, c.homo.data, 9);
	st.bundle.proj_method = ConnectedImages::flat;
	st.bundle.update_proj_range();
	HipCanvas blended(st.blend());
	put_canvas(fo, blended.get());
	HipCanvas pano(st.perspective_correction(blended.get()));
	blended.reset();
	put(fo, st.corners, 8);
	put(fo, st.inv, 9);
	put_canvas(fo, pano.get());
	fclose(fo);
	int h, w;
	PANO_HIP_CHECK(op_canvas_dims(pano.get(), &h, &w));
	fprintf(stderr, "Final Image Size: (%d, %d)\n", w, h);
	if (o.crop) {
		hip_crop_in_place(pano);
		PANO_HIP_CHECK(op_canvas_dims(pano.get(), &h, &w));
		fprintf(stderr, "Cropped Image Size: (%d, %d)\n", w, h);
	}
	write_files(o, pano.get());
	return 0;
}

// CylinderStitcher::build() as a client calls it: build(), the reference's own perspective_correction(Mat32f) on the blend
// that build left, then build_canvas(crop) on the same object for the files
static int run_cylinder_build(CylinderStitcher& st, const Options& o) {
	st.resident_views = o.resident;
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	Mat32f pano = st.build();
	put_mat(fo, pano);
	fprintf(stderr, "Final Image Size: (%d, %d)\n", pano.cols(), pano.rows());
	// the hook for the reference's source: a blended Mat32f in, the corrected one out
	put_mat(fo, hip_perspective_correction(st.bundle, hip_canvas_to_mat(HipCanvas(st.blend()))));
	op_ctx* ctx = HipContext::get();
	if (o.profile) { PANO_HIP_CHECK(op_ctx_set_profiling(ctx, 1)); PANO_HIP_CHECK(op_ctx_profile_reset(ctx)); }
	const auto t0 = std::chrono::steady_clock::now();
	HipCanvas cv(st.build_canvas(o.crop));
	PANO_HIP_CHECK(op_ctx_sync(ctx));
	const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (o.profile) {	// the context's stages (HIP events; those labelled "(host)" are host clocks), then their sums and the call's wall time
		double dev = 0, host = 0;
		for (int i = 0; i < op_ctx_profile_count(ctx); ++i) {
			const char* label; double ms; long calls;
			PANO_HIP_CHECK(op_ctx_profile_get(ctx, i, &label, &ms, &calls));
			fprintf(stderr, "profile: %.4f ms, %ld calls: %s\n", ms, calls, label);
			(std::string(label).find("(host)") == std::string::npos ? dev : host) += ms;
		}
		fprintf(stderr, "build_canvas: %.4f ms device stages, %.4f ms host stages, %.4f ms wall\n", dev, host, wall_ms);
		PANO_HIP_CHECK(op_ctx_set_profiling(ctx, 0));
	}
	put_canvas(fo, cv.get());
	fclose(fo);
	write_files(o, cv.get());
	return 0;
}

static int run_camera(Stitcher& st, const Options& o) { return o.mode == "camera_build" ? run_build(st, o) : run_camera_mode(st, o); }
static int run_cylinder(CylinderStitcher& st, const Options& o) { return o.mode == "cylinder_build" ? run_cylinder_build(st, o) : run_cylinder_mode(st, o); }

int main(int argc, char** argv) {
	Options o;
	HipCompensation& how = o.compensation;
	{	// --gain-compensation / --gain-blocks BXxBY may stand anywhere; the positional arguments keep their places
		int m = 1;
		for (int k = 1; k < argc; ++k) {
			if (std::string(argv[k]) == "--gain-compensation") how.gain = true;
			else if (std::string(argv[k]) == "--vignetting") how.vignetting = true;
			else if (std::string(argv[k]) == "--resident-views") o.resident = true;
			else if (std::string(argv[k]) == "--jpeg-list" && k + 1 < argc) { o.jpeg_list = argv[++k]; o.resident = true; }
			else if (std::string(argv[k]) == "--jpeg-orient") o.jpeg_orient = true;
			else if (std::string(argv[k]) == "--crop") o.crop = true;
			else if (std::string(argv[k]) == "--wrap") o.wrap = true;
			else if ((std::string(argv[k]) == "--planet" || std::string(argv[k]) == "--cube") && k + 1 < argc) {
				if (o.view != Options::NO_VIEW) { fprintf(stderr, "one of --planet, --view, --cube\n"); return 2; }
				o.view = std::string(argv[k]) == "--planet" ? Options::PLANET : Options::CUBE;
				if (sscanf(argv[++k], "%d", &o.view_n) != 1 || o.view_n < 1) { fprintf(stderr, "%s wants a size of at least 1; got %s\n", argv[k - 1], argv[k]); return 2; }
			}
			else if (std::string(argv[k]) == "--view" && k + 1 < argc) {
				if (o.view != Options::NO_VIEW) { fprintf(stderr, "one of --planet, --view, --cube\n"); return 2; }
				o.view = Options::LOOK;
				if (sscanf(argv[++k], "%lf,%lf,%lf,%lf,%dx%d", &o.look[0], &o.look[1], &o.look[2], &o.look[3], &o.view_w, &o.view_h) != 6) {
					fprintf(stderr, "--view wants YAW,PITCH,ROLL,HFOV,WxH; got %s\n", argv[k]); return 2;
				}
			}
			else if (std::string(argv[k]) == "--frame" && k + 1 < argc) {
				if (sscanf(argv[++k], "%lf,%lf,%lf,%lf", &o.frame[0], &o.frame[1], &o.frame[2], &o.frame[3]) != 4) {
					fprintf(stderr, "--frame wants LON0,LAT0,STEP_LON,STEP_LAT; got %s\n", argv[k]); return 2;
				}
				o.has_frame = true;
			}
			else if (std::string(argv[k]) == "--profile") o.profile = true;
			else if (std::string(argv[k]) == "--png" && k + 1 < argc) o.png_path = argv[++k];
			else if (std::string(argv[k]) == "--jpeg" && k + 1 < argc) o.jpeg_path = argv[++k];
			else if (std::string(argv[k]) == "--jpeg-444") o.jpeg_444 = true;
			else if (std::string(argv[k]) == "--jpeg-quality" && k + 1 < argc) {
				if (sscanf(argv[++k], "%d", &o.jpeg_quality) != 1 || o.jpeg_quality < 1 || o.jpeg_quality > 100) {
					fprintf(stderr, "--jpeg-quality wants an integer in [1, 100]; got %s\n", argv[k]); return 2;
				}
			}
			else if (std::string(argv[k]) == "--gain-blocks" && k + 1 < argc) {
				if (sscanf(argv[++k], "%dx%d", &how.bx, &how.by) != 2 || how.bx < 1 || how.bx > 16 || how.by < 1 || how.by > 16) {
					fprintf(stderr, "--gain-blocks wants BXxBY, each in [1, 16]; got %s\n", argv[k]); return 2;
				}
				how.gain = true;
			}
			else argv[m++] = argv[k];
		}
		argc = m;
	}
	if (how.vignetting && how.bx * how.by > 1) { fprintf(stderr, "--vignetting and --gain-blocks are exclusive\n"); return 2; }
	if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin [base_seed] [camera|camera_ordered|camera_build|cylinder|cylinder_build|reproject] [--gain-compensation] [--gain-blocks BXxBY] [--vignetting] [--png PATH] [--jpeg PATH] [--jpeg-quality Q] [--jpeg-444] [--resident-views] [--jpeg-list PATH [--jpeg-orient]] [--crop] [--profile] [--planet N | --view YAW,PITCH,ROLL,HFOV,WxH | --cube N] [--wrap] [--frame LON0,LAT0,STEP_LON,STEP_LAT]\n", argv[0]); return 2; }
	if (o.jpeg_orient && !o.jpeg_list) { fprintf(stderr, "--jpeg-orient goes with --jpeg-list\n"); return 2; }
	o.out_path = argv[2];
	o.base_seed = argc > 3 ? (uint32_t)strtoul(argv[3], nullptr, 10) : 42u;
	o.mode = argc > 4 ? argv[4] : "";
	const std::string& mode = o.mode;
	if (mode == "reproject") return run_reproject(argv[1], o);
	if (o.view != Options::NO_VIEW && mode != "camera_build") { fprintf(stderr, "--planet, --view and --cube go with reproject or camera_build\n"); return 2; }
	if ((o.wrap || o.has_frame) && o.view == Options::NO_VIEW) { fprintf(stderr, "--wrap and --frame go with --planet, --view or --cube\n"); return 2; }
	if (o.has_frame) { fprintf(stderr, "--frame goes with reproject: a build knows its own frame\n"); return 2; }
	const bool camera_mode = mode == "camera" || mode == "camera_ordered" || mode == "camera_build";
	config::ORDERED_INPUT = !camera_mode || mode == "camera_ordered"; config::ESTIMATE_CAMERA = camera_mode; config::TRANS = !camera_mode;   // TRANS mode: affine RANSAC, flat blend
	config::LAZY_READ = false;
	const bool cylinder_mode = mode == "cylinder" || mode == "cylinder_build";
	if (cylinder_mode) {
		if (how.gain || how.vignetting) { fprintf(stderr, "cylinder mode takes no gain or vignetting compensation\n"); return 2; }
		config::CYLINDER = true; config::ESTIMATE_CAMERA = false; config::TRANS = false; config::ORDERED_INPUT = true;
	}
	if (o.crop && !cylinder_mode) { fprintf(stderr, "--crop goes with cylinder\n"); return 2; }
	if (o.profile && mode != "cylinder_build") { fprintf(stderr, "--profile goes with cylinder_build\n"); return 2; }
	if (o.jpeg_list) {
		if (!camera_mode && !cylinder_mode) { fprintf(stderr, "--jpeg-list goes with camera, camera_ordered, camera_build or cylinder\n"); return 2; }
		std::vector<std::string> paths;
		FILE* fl = fopen(o.jpeg_list, "r");
		if (!fl) { perror(o.jpeg_list); return 2; }
		char line[4096];
		while (fgets(line, sizeof line, fl)) {
			std::string p(line);
			while (!p.empty() && (p.back() == '\n' || p.back() == '\r' || p.back() == ' ')) p.pop_back();
			if (!p.empty()) paths.push_back(p);
		}
		fclose(fl);
		if (cylinder_mode) {
			CylinderStitcher st(paths, o.base_seed, o.jpeg_orient);
			return run_cylinder(st, o);
		}
		Stitcher st(paths, o.base_seed, o.jpeg_orient);
		return run_camera(st, o);
	}
	FILE* fi = fopen(argv[1], "rb");
	if (!fi) { perror(argv[1]); return 2; }
	int32_t hdr[3];
	if (fread(hdr, 4, 3, fi) != 3) return 2;
	const int n = hdr[0], h = hdr[1], w = hdr[2];
	std::vector<Mat32f> mats;
	for (int k = 0; k < n; ++k) {
		mats.emplace_back(h, w, 3);
		if (fread(mats.back().ptr(), sizeof(float), (size_t)h * w * 3, fi) != (size_t)h * w * 3) return 2;
	}
	fclose(fi);
	if (cylinder_mode) {
		CylinderStitcher st(mats, o.base_seed);
		return run_cylinder(st, o);
	}
	if (camera_mode) {
		Stitcher st(mats, o.base_seed);
		return run_camera(st, o);
	}

	// ---- StitcherBase::calc_feature (stitch/stitcherbase.cc:9-27)
	std::vector<ImageRef> imgs;
	for (auto& m : mats) imgs.emplace_back(m);
	SIFTDetector feature_det;
	std::vector<const Mat32f*> ptrs;
	for (auto& r : imgs) ptrs.push_back(r.img);
	HipFeatureSet fs = feature_det.calc_feature(ptrs, o.resident);
	FILE* fo = fopen(o.out_path, "wb");
	if (!fo) { perror(o.out_path); return 2; }
	put_features(fo, fs);

	// ---- Stitcher::linear_pairwise_match (stitch/stitcher.cc:115-136): (i, i+1) for an ordered input
	std::vector<std::pair<int, int>> tasks;
	for (int i = 0; i + 1 < n; ++i) tasks.emplace_back(i, i + 1);
	std::vector<Shape2D> shapes;
	for (auto& r : imgs) shapes.push_back(r.shape());
	PairWiseMatcher pwmatcher(fs);
	pwmatcher.precompute(tasks);
	auto infos = hip_match_images(fs, shapes, tasks, o.base_seed);
	put_pairs(fo, pwmatcher, tasks, infos);

	// ---- chain to the middle image (stand-in for the host-only camera estimation), then
	// ConnectedImages::{calc_inverse_homo, update_proj_range, blend} (stitch/stitcher_image.cc)
	bool all = !tasks.empty();
	for (auto& r : infos) all = all && r.first;
	if (all) {
		ConnectedImages bundle;
		bundle.views = fs.views.get();                              // NULL without --resident-views
		bundle.proj_method = ConnectedImages::flat;
		bundle.identity_idx = n >> 1;                               // stitcher.cc:139
		std::vector<Homography> to_mid(n, Homography::I());
		for (int i = bundle.identity_idx + 1; i < n; ++i) to_mid[i] = to_mid[i - 1] * infos[i - 1].second.homo;     // H(i -> i-1)
		// images left of the middle need the inverse direction: invert through the C-ABI's host helper
		for (int i = bundle.identity_idx - 1; i >= 0; --i) {
			const op_config cfg = hip_config_snapshot();
			double hinv[9], rng[4]; op_blend_geom g; int sh[2] = {w, h};
			PANO_HIP_CHECK(op_blend_prepare(&cfg, 0, 0, 1, sh, infos[i].second.homo.data, &g, hinv, rng));
			Homography inv; for (int k = 0; k < 9; ++k) inv[k] = hinv[k];
			to_mid[i] = to_mid[i + 1] * inv;
		}
		for (int i = 0; i < n; ++i) {
			bundle.component.emplace_back(&imgs[i]);
			bundle.component.back().homo = to_mid[i];
		}
		bundle.calc_inverse_homo();
		bundle.update_proj_range();
		std::vector<float> gains;
		std::array<float, 3> poly;
		Mat32f pano = hip_compensate_and_blend(bundle, how, gains, poly);
		put_mat(fo, pano);
		for (auto& t : to_mid) put(fo, t.data, 9);
		put(fo, gains.data(), gains.size());
		if (how.vignetting) put(fo, poly.data(), 3);
		fprintf(stderr, "Final Image Size: (%d, %d)\n", pano.cols(), pano.rows());
		write_files(o, pano);
	} else {
		put1<int32_t>(fo, 0); put1<int32_t>(fo, 0);
	}
	fclose(fo);
	return 0;
}
