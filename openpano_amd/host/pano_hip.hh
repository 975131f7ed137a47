// pano_hip.hh -- C++ host mirror of the reference's class surface over the C-ABI
// (include/openpano_hip.h).  Header-only; link with -lopenpano_hip.
//
// Two build modes, same adapter code:
//   -DOPENPANO_WITH_REFERENCE (+ -I<reference>/src): the adapters are written against the
//        reference's OWN types (Mat32f, Descriptor, MatchData, MatchInfo, ConnectedImages, the
//        config:: globals) and plug into its class hierarchy -- HipSIFTDetector IS-A
//        pano::FeatureDetector, so `feature_det.reset(new HipSIFTDetector)` in
//        StitcherBase's constructor (stitch/stitcherbase.hh:53) is the whole integration for
//        SIFT.  INTEGRATION.md lists every such hook; oracle/ref_dropin_test.cc exercises them
//        against the reference's CPU classes in one process.
//   standalone: pano_types.hh supplies value types with the same names and members.
//
// Interfaces mirrored (file:line under /root/reference/src):
//   FeatureDetector::detect_feature / do_detect_feature   feature/feature.hh:42-57
//   StitcherBase::calc_feature (batched form)             stitch/stitcherbase.cc:9-27
//   PairWiseMatcher(feats).match(i, j)                    feature/matcher.hh:40-51
//   TransformEstimation(...).get_transform(MatchInfo*)    stitch/transform_estimate.hh:22-31
//   Stitcher::pairwise_match body (batched form)          stitch/stitcher.cc:66-136
//   ConnectedImages::blend                                stitch/stitcher_image.hh:92
//   CylinderWarper::warp                                  stitch/warp.hh:47-55
// Error behaviour follows the reference: unrecoverable conditions end in error_exit()
// (lib/debugutils.cc:57-60: message on stderr, exit(1)); no exception crosses the C-ABI.
//
// Layout, top down: errors, config snapshot, HipContext; the owning handles (HipFeatures .. HipJpeg: std::unique_ptr with the C
// entry's op_*_free as deleter, filled through hip_out); the helpers the adapters share, one copy of each (flattening, default
// task list, file reading, canvas -> Mat32f, crop in place; next to the blend: bundle / component geometry and
// hip_compensate_and_blend); the adapters in pipeline order (SIFT, MATCH, RANSAC, WARP + BLEND, the file writers); and, standalone
// only, HipStitcherBase with HipStitcher and HipCylinderStitcher derived from it.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <cstdlib>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "openpano_hip.h"

#ifdef OPENPANO_WITH_REFERENCE
#include "lib/config.hh"
#include "lib/mat.h"
#include "lib/geometry.hh"
#include "feature/feature.hh"
#include "feature/matcher.hh"
#include "stitch/match_info.hh"
#include "stitch/homography.hh"
#include "stitch/imageref.hh"
#include "stitch/stitcher_image.hh"
#include "stitch/camera.hh"
#include "lib/debugutils.hh"
#include "lib/timer.hh"
#include "pano_host.h"
#else
#include "pano_types.hh"
#include "pano_camera.hh"
#endif

namespace pano {

// ---- errors: the reference's error_exit (lib/debugutils.cc:57-60) ----
[[noreturn]] inline void hip_error_exit(const std::string& where) {
	fprintf(stderr, "%s: %s\n", where.c_str(), op_last_error());
	exit(1);
}
#define PANO_HIP_CHECK(expr) do { if ((expr) != OP_OK) ::pano::hip_error_exit(#expr); } while (0)

// ---- config: POD snapshot of namespace config at every call (the CLI fills the globals after
// static init, main.cc:237-292, so nothing is cached) ----
inline op_config hip_config_snapshot() {
	op_config c;
	op_config_default(&c);
	using namespace config;
	c.SIFT_WORKING_SIZE = SIFT_WORKING_SIZE; c.NUM_OCTAVE = NUM_OCTAVE; c.NUM_SCALE = NUM_SCALE;
	c.SCALE_FACTOR = SCALE_FACTOR; c.GAUSS_SIGMA = GAUSS_SIGMA; c.GAUSS_WINDOW_FACTOR = GAUSS_WINDOW_FACTOR;
	c.JUDGE_EXTREMA_DIFF_THRES = JUDGE_EXTREMA_DIFF_THRES; c.CONTRAST_THRES = CONTRAST_THRES;
	c.PRE_COLOR_THRES = PRE_COLOR_THRES; c.EDGE_RATIO = EDGE_RATIO;
	c.CALC_OFFSET_DEPTH = CALC_OFFSET_DEPTH; c.OFFSET_THRES = OFFSET_THRES;
	c.ORI_RADIUS = ORI_RADIUS; c.ORI_HIST_SMOOTH_COUNT = ORI_HIST_SMOOTH_COUNT;
	c.DESC_HIST_SCALE_FACTOR = DESC_HIST_SCALE_FACTOR; c.DESC_INT_FACTOR = DESC_INT_FACTOR;
	c.MATCH_REJECT_NEXT_RATIO = MATCH_REJECT_NEXT_RATIO;
	c.RANSAC_ITERATIONS = RANSAC_ITERATIONS; c.RANSAC_INLIER_THRES = RANSAC_INLIER_THRES;
	c.INLIER_IN_MATCH_RATIO = INLIER_IN_MATCH_RATIO; c.INLIER_IN_POINTS_RATIO = INLIER_IN_POINTS_RATIO;
	c.CYLINDER = CYLINDER; c.TRANS = TRANS; c.ESTIMATE_CAMERA = ESTIMATE_CAMERA;
	c.ORDERED_INPUT = ORDERED_INPUT; c.LAZY_READ = LAZY_READ; c.MULTIBAND = MULTIBAND;
	c.MAX_OUTPUT_SIZE = MAX_OUTPUT_SIZE; c.FOCAL_LENGTH = FOCAL_LENGTH;
	return c;
}

// ---- one op_ctx per host thread: the reference calls detect_feature / match concurrently from
// OpenMP threads (stitcherbase.cc:14, stitcher.cc:106); contexts are thread-compatible ----
class HipContext {
	public:
		static op_ctx* get() {
			thread_local HipContext c;
			return c.ctx;
		}
		static int& device() { static int d = 0; return d; }     // set before first use to pick a GPU
		// Several GPUs in this process: set_devices({0, 1, ...}) -- or OPENPANO_DEVICES=0,1,... in
		// the environment -- makes the batched adapters (HipSIFTDetector::calc_feature, HipPairWiseMatcher)
		// shard their image / pair loops over the listed devices; results land on the first one.
		static void set_devices(const std::vector<int>& devs) {
			if (group_slot()) { op_group_destroy(group_slot()); group_slot() = nullptr; }
			if (devs.size() > 1) PANO_HIP_CHECK(op_group_create(devs.data(), (int)devs.size(), &group_slot()));
			if (!devs.empty()) device() = devs[0];
			group_env_done() = true;
		}
		static op_group* group() {
			if (!group_env_done()) {
				group_env_done() = true;
				if (const char* e = std::getenv("OPENPANO_DEVICES")) {
					std::vector<int> devs;
					for (const char* p = e; *p;) { devs.push_back(atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
					set_devices(devs);
				}
			}
			return group_slot();
		}
		// the context that owns gathered results: context 0 of the group, else this thread's own
		static op_ctx* home() { return group() ? op_group_ctx(group(), 0) : get(); }
	private:
		static op_group*& group_slot() { static op_group* g = nullptr; return g; }
		static bool& group_env_done() { static bool b = false; return b; }
		op_ctx* ctx = nullptr;
		HipContext() { PANO_HIP_CHECK(op_ctx_create(device(), nullptr, &ctx)); }
		~HipContext() { op_ctx_destroy(ctx); }
};

// ---- owning handles: what a C entry handed out, released through that entry's op_*_free when its owner goes.  Functions
// that hand a handle on to their caller return the raw pointer (release()) ----
template <typename T, void (*Free)(T*)>
struct HipFree { void operator()(T* p) const { Free(p); } };
template <typename T, void (*Free)(T*)>
using HipHandle = std::unique_ptr<T, HipFree<T, Free>>;
using HipFeatures = HipHandle<op_features, op_features_free>;
using HipViews = HipHandle<op_views, op_views_free>;
using HipMatches = HipHandle<op_matches, op_matches_free>;
using HipRansac = HipHandle<op_ransac_result, op_ransac_free>;
using HipCanvas = HipHandle<op_canvas, op_canvas_free>;
using HipPng = HipHandle<op_png, op_png_free>;
using HipJpeg = HipHandle<op_jpeg, op_jpeg_free>;
// hip_out(h): the T** a C entry writes its result through; h adopts what was written when the call's statement ends
template <typename H>
struct HipOut {
	H& h;
	typename H::pointer p = nullptr;
	operator typename H::pointer*() { return &p; }
	~HipOut() { h.reset(p); }
};
template <typename H> inline HipOut<H> hip_out(H& h) { return {h}; }

// ---- the lists the C-ABI takes flat ----
// Vec2D list <-> x, y doubles
inline std::vector<double> hip_flatten(const std::vector<Vec2D>& pts) {
	std::vector<double> p(pts.size() * 2 + 2);
	for (size_t i = 0; i < pts.size(); ++i) { p[2 * i] = pts[i].x; p[2 * i + 1] = pts[i].y; }
	return p;
}
inline void hip_unflatten(const std::vector<double>& p, std::vector<Vec2D>& pts) {
	for (size_t i = 0; i < pts.size(); ++i) pts[i] = Vec2D(p[2 * i], p[2 * i + 1]);
}
// (i, j) pairs -> i, j ints; shapes -> w, h ints
inline std::vector<int> hip_flatten(const std::vector<std::pair<int, int>>& pairs) {
	std::vector<int> pr;
	for (auto& t : pairs) { pr.push_back(t.first); pr.push_back(t.second); }
	return pr;
}
inline std::vector<int> hip_flatten(const std::vector<Shape2D>& shapes) {
	std::vector<int> sh;
	for (auto& s : shapes) { sh.push_back(s.w); sh.push_back(s.h); }
	return sh;
}
// the coordinates of a descriptor list (StitcherBase::keypoints, stitcherbase.cc:23-25)
inline std::vector<Vec2D> hip_keypoints(const std::vector<Descriptor>& feats) {
	std::vector<Vec2D> kps;
	kps.reserve(feats.size());
	for (auto& d : feats) kps.emplace_back(d.coor);
	return kps;
}
// coordinates-only features (no descriptors: RANSAC reads nothing else) from one keypoint list per view
inline HipFeatures hip_features_from_keypoints(op_ctx* ctx, const std::vector<const std::vector<Vec2D>*>& kpts) {
	std::vector<std::vector<double>> flat;
	std::vector<const double*> cp; std::vector<int> counts;
	for (auto* k : kpts) { flat.push_back(hip_flatten(*k)); counts.push_back((int)k->size()); }
	for (auto& f : flat) cp.push_back(f.data());
	HipFeatures f;
	PANO_HIP_CHECK(op_features_from_host(ctx, nullptr, cp.data(), counts.data(), (int)kpts.size(), hip_out(f)));
	return f;
}
// the default task list of Stitcher::pairwise_match (all i < j, stitcher.cc:99-100) or, for an ordered input, of
// linear_pairwise_match ((i, i + 1 mod n), stitcher.cc:121-124)
inline std::vector<std::pair<int, int>> hip_default_tasks(int n, bool ordered) {
	std::vector<std::pair<int, int>> tasks;
	if (ordered) for (int i = 0; i < n; ++i) tasks.emplace_back(i, (i + 1) % n);
	else for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) tasks.emplace_back(i, j);
	return tasks;
}
// the bytes of a file, all of them or the first `limit`; a file that cannot be opened ends the program like read_img
// (lib/imgio.cc:68-69)
inline std::vector<unsigned char> hip_read_file(const std::string& path, size_t limit = (size_t)-1) {
	FILE* f = fopen(path.c_str(), "rb");
	if (!f) { fprintf(stderr, "File \"%s\" not exists!\n", path.c_str()); exit(1); }
	std::vector<unsigned char> data;
	unsigned char buf[65536]; size_t n;
	data.reserve(std::min(sizeof buf, limit));      // data() of an empty file is not NULL either
	while (data.size() < limit && (n = fread(buf, 1, std::min(sizeof buf, limit - data.size()), f)) > 0) data.insert(data.end(), buf, buf + n);
	fclose(f);
	return data;
}

// ---- canvases ----
// the pixels of a device canvas as a matrix in host memory; the canvas is released
inline Mat32f hip_canvas_to_mat(HipCanvas cv) {
	int h, w;
	PANO_HIP_CHECK(op_canvas_dims(cv.get(), &h, &w));
	Mat32f out(h, w, 3);
	PANO_HIP_CHECK(op_canvas_copy(HipContext::get(), cv.get(), out.ptr()));
	cv.reset();     // here, not where the caller's full expression ends
	return out;
}
// crop() (lib/imgproc.cc:200-235) on the device: cv becomes its largest valid rectangle, the uncropped canvas is released
inline void hip_crop_in_place(HipCanvas& cv) {
	HipCanvas cropped;
	PANO_HIP_CHECK(op_canvas_crop(HipContext::get(), cv.get(), hip_out(cropped), nullptr, nullptr));
	cv = std::move(cropped);
}

// ===================================== SIFT =====================================
#ifndef OPENPANO_WITH_REFERENCE
// the reference's base class (feature/feature.hh:42-52): detect_feature re-centres the [0,1)
// coordinates do_detect_feature returns (feature/feature.cc:20-28)
class FeatureDetector {
	public:
		FeatureDetector() = default;
		virtual ~FeatureDetector() = default;
		FeatureDetector(const FeatureDetector&) = delete;
		FeatureDetector& operator=(const FeatureDetector&) = delete;
		std::vector<Descriptor> detect_feature(const Mat32f& img) const {
			auto ret = do_detect_feature(img);
			for (auto& d : ret) {
				d.coor.x = (d.coor.x - 0.5) * img.width();
				d.coor.y = (d.coor.y - 0.5) * img.height();
			}
			return ret;
		}
		virtual std::vector<Descriptor> do_detect_feature(const Mat32f& img) const = 0;
};
#endif

// device-resident features of a whole image set: what StitcherBase keeps as `feats`, plus the
// op_features handle so that the matcher does not re-upload descriptors
struct HipFeatureSet {
	HipFeatures handle;
	// the images themselves, resident on the device in the type they were uploaded in (calc_feature with resident_views):
	// the blend and the overlap passes read them there instead of a second, fp32 upload (ConnectedImages::views)
	HipViews views;
	std::vector<std::vector<Descriptor>> feats;     // centred coordinates, like StitcherBase::feats
	HipFeatureSet() = default;
	HipFeatureSet(HipFeatureSet&&) = default;
	HipFeatureSet& operator=(HipFeatureSet&&) = default;
	~HipFeatureSet() { handle.reset(); }            // the features go before the views, as in a move assignment
};

class HipSIFTDetector : public FeatureDetector {
	public:
		// SIFTDetector::do_detect_feature (feature/feature.cc:31-47): [0,1) coordinates
		std::vector<Descriptor> do_detect_feature(const Mat32f& mat) const override {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			op_image im{mat.ptr(), mat.rows(), mat.cols(), 0, OP_F32};
			if (mat.channels() != 3) { fprintf(stderr, "HipSIFTDetector: image must have 3 channels\n"); exit(1); }
			HipFeatures own;
			PANO_HIP_CHECK(op_sift_batch(ctx, &cfg, &im, 1, hip_out(own)));
			const op_features* f = own.get();
			const int k = op_features_count(f, 0);
			std::vector<float> desc((size_t)k * 128);
			std::vector<double> real((size_t)k * 2);
			if (k) {
				PANO_HIP_CHECK(op_features_copy(ctx, f, 0, desc.data(), nullptr));
				PANO_HIP_CHECK(op_features_copy_real(ctx, f, 0, real.data()));
			}
			own.reset();
			std::vector<Descriptor> ret(k);
			for (int i = 0; i < k; ++i) {
				ret[i].coor = Vec2D(real[2 * i], real[2 * i + 1]);
				ret[i].descriptor.assign(desc.begin() + (size_t)i * 128, desc.begin() + (size_t)(i + 1) * 128);
			}
			return ret;
		}

		// StitcherBase::calc_feature (stitch/stitcherbase.cc:9-27) as ONE batched device call:
		// all images in one launch series, descriptors left resident for the matcher.
		// resident_views: the images go up ONCE as an op_views kept in the result (bytes when every pixel is an exact k / 255,
		// fp32 otherwise), SIFT reads them there, and so do the blend and the overlap passes of a bundle whose `views` is set
		// to it.  Ignored with a device group, whose images are dealt over several GPUs.
		HipFeatureSet calc_feature(const std::vector<const Mat32f*>& imgs, bool resident_views = false) const {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			std::vector<op_image> ims;
			for (auto* m : imgs) ims.push_back(op_image{m->ptr(), m->rows(), m->cols(), 0, OP_F32});
			// Images that came out of a decoder are bytes / 255 (read_img, lib/imgio.cc:54-56,75-77: (float)((double)byte / 255.0)).
			// When EVERY value of every image is exactly such a float, the bytes travel instead -- a quarter of the PCIe traffic,
			// pageable memory at that -- and the device converts them with the same expression (OP_U8): the same features, bit for bit.
			// Non-decoder inputs (warped, normalised images) must not pay for this: a probe of every image's first values decides
			// whether the byte buffers are allocated at all, the full scan stops at the first chunk that holds a mismatch, and
			// the comparison is on BIT PATTERNS (-0.0f is not the float of byte 0).
			std::vector<std::unique_ptr<unsigned char[]>> bytes(imgs.size());
			if (!HipContext::group()) {
				auto as_byte = [](float v, unsigned char& b) {
					const float q = v * 255.f + 0.5f;
					const int c = q >= 0.f && q < 256.f ? (int)q : 0;
					b = (unsigned char)c;
					const float back = (float)((double)c / 255.0);
					uint32_t x, y; memcpy(&x, &back, 4); memcpy(&y, &v, 4);
					return x == y;
				};
				bool plausible = true;
				for (size_t k = 0; k < imgs.size() && plausible; ++k) {
					const size_t n = std::min<size_t>((size_t)imgs[k]->rows() * imgs[k]->cols() * 3, 4096);
					const float* v = imgs[k]->ptr();
					unsigned char b;
					for (size_t e = 0; e < n && plausible; ++e) plausible = as_byte(v[e], b);
				}
				std::atomic<int> all_bytes{plausible ? 1 : 0};
				if (plausible) {
					for (size_t k = 0; k < imgs.size(); ++k) bytes[k].reset(new unsigned char[(size_t)imgs[k]->rows() * imgs[k]->cols() * 3]);
#pragma omp parallel for schedule(dynamic)
					for (long job = 0; job < (long)imgs.size() * 8; ++job) {
						const size_t k = (size_t)(job >> 3), part = (size_t)(job & 7), n = (size_t)imgs[k]->rows() * imgs[k]->cols() * 3;
						const float* v = imgs[k]->ptr();
						unsigned char* b = bytes[k].get();
						const size_t e1 = n * (part + 1) / 8;
						for (size_t e0 = n * part / 8; e0 < e1 && all_bytes.load(std::memory_order_relaxed); e0 += 65536) {
							bool ok = true;
							for (size_t e = e0; e < std::min(e1, e0 + 65536); ++e) ok &= as_byte(v[e], b[e]);
							if (!ok) all_bytes.store(0, std::memory_order_relaxed);
						}
					}
				}
				if (all_bytes.load()) for (size_t k = 0; k < imgs.size(); ++k) { ims[k].data = bytes[k].get(); ims[k].dtype = OP_U8; }
			}
			if (op_group* g = HipContext::group()) {        // images dealt over the group's GPUs, features all-gathered
				HipFeatureSet fs;
				PANO_HIP_CHECK(op_sift_batch_multi(g, &cfg, ims.data(), (int)ims.size(), hip_out(fs.handle)));
				fetch_feats(op_group_ctx(g, 0), fs, imgs.size());
				return fs;
			}
			if (resident_views) {       // one upload, then as for views that are on the device already
				HipViews views;
				PANO_HIP_CHECK(op_views_upload(ctx, ims.data(), (int)ims.size(), hip_out(views)));
				return calc_feature(views.release());
			}
			// uploads, kernels and the copy back to the host pipelined over chunks of the batch; the host buffers are
			// sized from a first guess and the call repeated once if the images hold more features than that
			HipFeatureSet fs;
			std::vector<float> desc; std::vector<double> coor;
			size_t cap = (size_t)imgs.size() * 4096;
			for (int attempt = 0; attempt < 2; ++attempt) {
				desc.resize(cap * 128 + 1); coor.resize(cap * 2 + 1);
				const int rc = op_sift_batch_host(ctx, &cfg, ims.data(), (int)ims.size(), desc.data(), coor.data(), (int64_t)cap, hip_out(fs.handle));
				if (rc == OP_OK) break;
				if (rc != OP_ERR_CAPACITY || attempt == 1) hip_error_exit("op_sift_batch_host");
				cap = (size_t)op_features_total(fs.handle.get()) + 16;
				fs.handle.reset();
			}
			fill_feats(fs, imgs.size(), desc, coor);
			return fs;
		}

		// The same for views that are already on the device -- decoded there by hip_read_jpeg_views, or uploaded by the
		// caller: no host pixel is read.  The result owns `views` (HipFeatureSet::views), as calc_feature(imgs, true) owns its upload.
		HipFeatureSet calc_feature(op_views* views) const {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			HipFeatureSet fs;
			fs.views.reset(views);
			const int n = op_views_count(views);
			if (n <= 0) hip_error_exit("calc_feature(op_views*)");
			std::vector<op_image> dev((size_t)n);
			for (int k = 0; k < n; ++k) PANO_HIP_CHECK(op_views_image(views, k, &dev[k]));
			PANO_HIP_CHECK(op_sift_batch(ctx, &cfg, dev.data(), n, hip_out(fs.handle)));
			fetch_feats(ctx, fs, (size_t)n);
			return fs;
		}

	private:
		// every image's descriptors and coordinates from the device handle into fs.feats
		static void fetch_feats(op_ctx* ctx, HipFeatureSet& fs, size_t nimg) {
			const op_features* f = fs.handle.get();
			const size_t total = (size_t)op_features_total(f);
			std::vector<float> desc(total * 128 + 1); std::vector<double> coor(total * 2 + 1);
			for (int k = 0; k < (int)nimg; ++k)
				if (op_features_count(f, k))
					PANO_HIP_CHECK(op_features_copy(ctx, f, k, desc.data() + (size_t)op_features_offset(f, k) * 128, coor.data() + (size_t)op_features_offset(f, k) * 2));
			fill_feats(fs, nimg, desc, coor);
		}
		static void fill_feats(HipFeatureSet& fs, size_t nimg, const std::vector<float>& desc, const std::vector<double>& coor) {
			const op_features* f = fs.handle.get();
			fs.feats.resize(nimg);
			for (size_t k = 0; k < nimg; ++k) {
				const int n = op_features_count(f, (int)k);
				if (n == 0) {    // stitcherbase.cc:20-21
					fprintf(stderr, "Cannot find feature in image %d!\n", (int)k);
					exit(1);
				}
				const float* d = desc.data() + (size_t)op_features_offset(f, (int)k) * 128;
				const double* c = coor.data() + (size_t)op_features_offset(f, (int)k) * 2;
				fs.feats[k].resize(n);
				for (int i = 0; i < n; ++i) {
					fs.feats[k][i].coor = Vec2D(c[2 * i], c[2 * i + 1]);
					fs.feats[k][i].descriptor.assign(d + (size_t)i * 128, d + (size_t)(i + 1) * 128);
				}
			}
		}
};

// ImageRef::load for a job of baseline JPEG files (stitch/imageref.hh:22-27 -> read_img, lib/imgio.cc:67-90): the files are
// read, their headers parsed on the host, and everything else -- Huffman decode, IDCT, upsampling, colour -- runs on the
// device (op_views_decode_jpeg).  The views are bytes, every one of them libjpeg's; the caller owns the result
// (op_views_free), or hands it to HipSIFTDetector::calc_feature(op_views*).  A file outside the format ends the program with
// the library's message, which names its index; op_jpeg_probe tells beforehand.
// orient: every view turned upright by its file's EXIF orientation (op_views_decode_jpeg_oriented), which the reference's
// decoder ignores; a view of orientation 5..8 is then w x h.
inline op_views* hip_read_jpeg_views(op_ctx* ctx, const std::vector<std::string>& paths, bool orient = false) {
	std::vector<std::vector<unsigned char>> data(paths.size());
	std::vector<const unsigned char*> ptr(paths.size());
	std::vector<int64_t> size(paths.size());
	for (size_t k = 0; k < paths.size(); ++k) {
		data[k] = hip_read_file(paths[k]);
		ptr[k] = data[k].empty() ? nullptr : data[k].data(); size[k] = (int64_t)data[k].size();     // an empty file is refused as NULL data
	}
	op_views* v = nullptr;
	if (orient) PANO_HIP_CHECK(op_views_decode_jpeg_oriented(ctx, ptr.data(), size.data(), (int)paths.size(), nullptr, &v));
	else PANO_HIP_CHECK(op_views_decode_jpeg(ctx, ptr.data(), size.data(), (int)paths.size(), &v));
	return v;
}

// The EXIF orientation (1..8; 1 when absent or unreadable) and FocalLengthIn35mmFilm (mm; 0 when absent) of a camera file
// (op_jpeg_exif) -- the latter is what config.cfg's FOCAL_LENGTH asks the user for.  Either pointer may be NULL.  EXIF sits in
// front of the tables, so the first megabyte of the file is all that is read.
inline void hip_jpeg_exif(const std::string& path, int* orientation, int* focal35) {
	const std::vector<unsigned char> head = hip_read_file(path, 1 << 20);
	PANO_HIP_CHECK(op_jpeg_exif(head.data(), (int64_t)head.size(), orientation, focal35));
}

// ===================================== MATCH =====================================
// Same public signature as the reference's PairWiseMatcher (feature/matcher.hh:40-51).  match()
// may be called concurrently (stitcher.cc:106-109): the first call matches the whole task list
// in one device launch series, later calls are lookups.
class HipPairWiseMatcher {
	public:
		explicit HipPairWiseMatcher(const std::vector<std::vector<Descriptor>>& feats): feats(feats) {
			if (feats.empty() || feats.at(0).empty()) { fprintf(stderr, "PairWiseMatcher: no features\n"); exit(1); }
			upload();
		}
		// descriptors already resident (HipSIFTDetector::calc_feature): no second H2D pass
		explicit HipPairWiseMatcher(const HipFeatureSet& fs): feats(fs.feats), handle(fs.handle.get()), owns(false) {}
		HipPairWiseMatcher(const HipPairWiseMatcher&) = delete;
		HipPairWiseMatcher& operator=(const HipPairWiseMatcher&) = delete;
		~HipPairWiseMatcher() { if (owns) op_features_free(handle); }

		// return pair of <idx in i, idx in j>
		MatchData match(int i, int j) const {
			std::lock_guard<std::mutex> lk(mu);
			if (cache.empty()) precompute_default();
			auto it = cache.find(std::make_pair(i, j));
			if (it == cache.end()) {
				run({{i, j}});
				it = cache.find(std::make_pair(i, j));
			}
			return it->second;
		}

		// match an explicit task list in one call (Stitcher::pairwise_match's `tasks`)
		void precompute(const std::vector<std::pair<int, int>>& tasks) const {
			std::lock_guard<std::mutex> lk(mu);
			run(tasks);
		}
		op_features* device_features() const { return handle; }

	protected:
		const std::vector<std::vector<Descriptor>>& feats;    // must outlive the matcher (matcher.hh:59)
		op_features* handle = nullptr;
		bool owns = true;
		mutable std::mutex mu;
		mutable std::map<std::pair<int, int>, MatchData> cache;

		void upload() {
			const int n = (int)feats.size();
			std::vector<std::vector<float>> flat(n);
			std::vector<std::vector<double>> coor(n);
			std::vector<const float*> dp(n); std::vector<const double*> cp(n); std::vector<int> counts(n);
			for (int k = 0; k < n; ++k) {       // PairWiseMatcher::build flattening (matcher.cc:75-81)
				counts[k] = (int)feats[k].size();
				flat[k].resize((size_t)counts[k] * 128 + 1);
				for (int i = 0; i < counts[k]; ++i) {
					if (feats[k][i].descriptor.size() != 128) { fprintf(stderr, "PairWiseMatcher: descriptors must be 128-D\n"); exit(1); }
					memcpy(&flat[k][(size_t)i * 128], feats[k][i].descriptor.data(), 128 * sizeof(float));
				}
				coor[k] = hip_flatten(hip_keypoints(feats[k]));
				dp[k] = flat[k].data(); cp[k] = coor[k].data();
			}
			PANO_HIP_CHECK(op_features_from_host(HipContext::home(), dp.data(), cp.data(), counts.data(), n, &handle));
		}
		void precompute_default() const { run(hip_default_tasks((int)feats.size(), config::ORDERED_INPUT)); }
		void run(const std::vector<std::pair<int, int>>& tasks) const {
			if (tasks.empty()) return;
			const std::vector<int> pr = hip_flatten(tasks);
			const op_config cfg = hip_config_snapshot();
			HipMatches own;
			if (op_group* g = HipContext::group())          // pair list dealt over the group's GPUs (K_i * K_j balanced)
				PANO_HIP_CHECK(op_match_pairs_multi(g, &cfg, handle, pr.data(), (int)tasks.size(), hip_out(own)));
			else
				PANO_HIP_CHECK(op_match_pairs(HipContext::get(), &cfg, handle, pr.data(), (int)tasks.size(), hip_out(own)));
			const op_matches* m = own.get();
			for (size_t p = 0; p < tasks.size(); ++p) {
				const int c = op_matches_count(m, (int)p);
				std::vector<int> idx((size_t)c * 2 + 2);
				if (c) PANO_HIP_CHECK(op_matches_copy(m, (int)p, idx.data()));
				MatchData md;
				for (int q = 0; q < c; ++q) md.data.emplace_back(idx[2 * q], idx[2 * q + 1]);
				cache[tasks[p]] = std::move(md);
			}
		}
};

// ===================================== RANSAC =====================================
// Same constructor and get_transform as the reference's TransformEstimation
// (stitch/transform_estimate.hh:22-31).  The reference seeds std::mt19937 from
// std::random_device per call (transform_estimate.cc:64-65); so does this adapter unless a seed
// is injected (tests, reproducible runs).
class HipTransformEstimation {
	public:
		HipTransformEstimation(const MatchData& m_match, const std::vector<Vec2D>& kp1, const std::vector<Vec2D>& kp2,
				const Shape2D& shape1, const Shape2D& shape2):
			match(m_match), kp1(kp1), kp2(kp2), shape1(shape1), shape2(shape2) {}
		HipTransformEstimation(const HipTransformEstimation&) = delete;
		HipTransformEstimation& operator=(const HipTransformEstimation&) = delete;

		static bool& seed_injected() { static bool b = false; return b; }
		static uint32_t& injected_seed() { static uint32_t s = 0; return s; }

		// get a transform matrix from second(f2) -> first(f1)
		bool get_transform(MatchInfo* info) {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			const HipFeatures f = hip_features_from_keypoints(ctx, {&kp1, &kp2});
			std::vector<int> idx = hip_flatten(match.data);
			idx.resize(idx.size() + 2);
			const int* ip[1] = {idx.data()};
			const int mc[1] = {(int)match.data.size()};
			HipMatches m;
			PANO_HIP_CHECK(op_matches_from_host(ip, mc, 1, hip_out(m)));
			const int pairs[2] = {0, 1};
			const int shapes[4] = {shape1.w, shape1.h, shape2.w, shape2.h};
			uint32_t seed = seed_injected() ? injected_seed() : std::random_device{}();
			HipRansac r;
			PANO_HIP_CHECK(op_ransac_pairs(ctx, &cfg, f.get(), m.get(), pairs, 1, shapes, &seed, 0, hip_out(r)));
			return fill(r.get(), 0, match, kp1, kp2, info);
		}

		// MatchInfo of pair p of a batched result (fill_inliers_to_matchinfo's outputs,
		// transform_estimate.cc:150-218)
		static bool fill(const op_ransac_result* r, int p, const MatchData& match, const std::vector<Vec2D>& kp1,
				const std::vector<Vec2D>& kp2, MatchInfo* info) {
			info->confidence = op_ransac_confidence(r, p);
			if (!op_ransac_ok(r, p)) return false;
			double h[9];
			PANO_HIP_CHECK(op_ransac_homo(r, p, h));
			for (int i = 0; i < 9; ++i) info->homo[i] = h[i];
			const int n = op_ransac_inlier_count(r, p);
			std::vector<int> inl(n + 1);
			if (n) PANO_HIP_CHECK(op_ransac_inliers(r, p, inl.data()));
			info->match.clear();
			for (int i = 0; i < n; ++i)
				info->match.emplace_back(kp1[match.data[inl[i]].first], kp2[match.data[inl[i]].second]);
			return true;
		}

	private:
		const MatchData& match;
		const std::vector<Vec2D>&kp1, &kp2;
		const Shape2D shape1, shape2;
};

// One op_match_pairs + one op_ransac_pairs for a whole task list; pair p's RANSAC seed is seeds[p] (or derived from
// base_seed and p when seeds is empty).  The match lists never leave the device between the two calls; they come
// to the host once, for MatchInfo::match and the caller's MatchData.
inline void hip_match_and_estimate(const HipFeatureSet& fs, const std::vector<Shape2D>& shapes, const std::vector<std::pair<int, int>>& tasks,
		const std::vector<uint32_t>& seeds, uint32_t base_seed, std::vector<MatchData>& matches, std::vector<std::pair<bool, MatchInfo>>& out) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	const std::vector<int> pr = hip_flatten(tasks), sh = hip_flatten(shapes);
	const op_features* f = fs.handle.get();
	const uint32_t* sd = seeds.empty() ? nullptr : seeds.data();
	HipMatches m;
	HipRansac r;
	if (op_group* g = HipContext::group()) {           // pair list dealt over the group's GPUs; RANSAC follows the deal
		PANO_HIP_CHECK(op_match_pairs_multi(g, &cfg, f, pr.data(), (int)tasks.size(), hip_out(m)));
		PANO_HIP_CHECK(op_ransac_pairs_multi(g, &cfg, f, m.get(), pr.data(), (int)tasks.size(), sh.data(), sd, base_seed, hip_out(r)));
	} else {
		PANO_HIP_CHECK(op_match_pairs(ctx, &cfg, f, pr.data(), (int)tasks.size(), hip_out(m)));
		PANO_HIP_CHECK(op_ransac_pairs(ctx, &cfg, f, m.get(), pr.data(), (int)tasks.size(), sh.data(), sd, base_seed, hip_out(r)));
	}
	std::vector<int64_t> off(tasks.size() + 1);
	std::vector<int> idx((size_t)op_matches_total(m.get()) * 2 + 2);
	PANO_HIP_CHECK(op_matches_copy_all(m.get(), idx.data(), off.data()));
	matches.assign(tasks.size(), MatchData());
	out.assign(tasks.size(), std::pair<bool, MatchInfo>());
	std::vector<std::vector<Vec2D>> kps;
	for (auto& fk : fs.feats) kps.push_back(hip_keypoints(fk));
	for (size_t p = 0; p < tasks.size(); ++p) {
		MatchData& md = matches[p];
		md.data.reserve((size_t)(off[p + 1] - off[p]));
		for (int64_t q = off[p]; q < off[p + 1]; ++q) md.data.emplace_back(idx[2 * q], idx[2 * q + 1]);
		out[p].first = HipTransformEstimation::fill(r.get(), (int)p, md, kps[tasks[p].first], kps[tasks[p].second], &out[p].second);
	}
}

// ---- the batched hooks inside the reference's OWN loops ("batched form") ----
// Stitcher::pairwise_match / linear_pairwise_match (stitch/stitcher.cc:96-136) construct one matcher and then call
// match_image(pwmatcher, i, j) per task from an OpenMP loop; match_image (:66-94) asks the matcher for the pair's
// MatchData, runs a TransformEstimation on it and keeps the bookkeeping.  HipBatchedMatcher has PairWiseMatcher's
// place and match(i, j) signature, but its constructor runs the WHOLE default task list (all i < j, or (i, i + 1)
// under ORDERED_INPUT: the lists of :99-100 / :121-124) through one op_match_pairs + one op_ransac_pairs; match()
// returns a MatchData that remembers where its pair's RANSAC result lies, and HipBatchedTransformEstimation -- in
// TransformEstimation's place, same constructor and get_transform -- hands that result over.  The reference's loop
// bodies stay as they are.
struct HipMatchData : public MatchData {
	const std::pair<bool, MatchInfo>* estimated = nullptr;
};
class HipBatchedMatcher {
	public:
		// imgs: anything with shape() per image (std::vector<ImageRef>, stitcherbase.hh:28)
		template <typename ImageList>
		HipBatchedMatcher(const HipFeatureSet& fs, const ImageList& imgs): tasks(hip_default_tasks((int)fs.feats.size(), config::ORDERED_INPUT)) {
			std::vector<Shape2D> shapes;
			for (auto& r : imgs) shapes.push_back(r.shape());
			// the reference seeds every get_transform from std::random_device (transform_estimate.cc:64-65)
			std::vector<uint32_t> seeds(tasks.size());
			for (auto& s : seeds) s = HipTransformEstimation::seed_injected() ? HipTransformEstimation::injected_seed() : std::random_device{}();
			hip_match_and_estimate(fs, shapes, tasks, seeds, 0, matches, results);
			for (size_t p = 0; p < tasks.size(); ++p) index[tasks[p]] = p;
		}
		HipBatchedMatcher(const HipBatchedMatcher&) = delete;
		HipBatchedMatcher& operator=(const HipBatchedMatcher&) = delete;
		// return pair of <idx in i, idx in j>, plus the pair's transform estimate
		HipMatchData match(int i, int j) const {
			auto it = index.find(std::make_pair(i, j));
			if (it == index.end()) { fprintf(stderr, "HipBatchedMatcher: pair (%d, %d) is not in the task list\n", i, j); exit(1); }
			HipMatchData md;
			md.data = matches[it->second].data;
			md.estimated = &results[it->second];
			return md;
		}
	private:
		std::vector<std::pair<int, int>> tasks;
		std::vector<MatchData> matches;
		std::vector<std::pair<bool, MatchInfo>> results;
		std::map<std::pair<int, int>, size_t> index;
};
class HipBatchedTransformEstimation {
	public:
		HipBatchedTransformEstimation(const HipMatchData& m_match, const std::vector<Vec2D>&, const std::vector<Vec2D>&, const Shape2D&, const Shape2D&):
			match(m_match) {}
		bool get_transform(MatchInfo* info) {
			*info = match.estimated->second;
			return match.estimated->first;
		}
	private:
		const HipMatchData& match;
};

// Body of Stitcher::pairwise_match / linear_pairwise_match + match_image (stitch/stitcher.cc:66-136)
// for a whole task list: ONE matcher call and ONE batched RANSAC call.  out[k] = (succ, info of
// tasks[k], homography from j to i) -- the caller keeps the reference's bookkeeping
// (pairwise_matches[i][j] / inverse for [j][i], stitcher.cc:79-93).
inline std::vector<std::pair<bool, MatchInfo>> hip_match_images(const HipFeatureSet& fs,
		const std::vector<Shape2D>& shapes, const std::vector<std::pair<int, int>>& tasks, uint32_t base_seed) {
	std::vector<MatchData> matches;
	std::vector<std::pair<bool, MatchInfo>> out;
	hip_match_and_estimate(fs, shapes, tasks, std::vector<uint32_t>(), base_seed, matches, out);
	return out;
}

// ===================================== WARP + BLEND =====================================
#ifndef OPENPANO_WITH_REFERENCE
// stitch/stitcher_image.hh:15-98 (fields and method names as in the reference)
struct ConnectedImages {
	ConnectedImages() = default;
	ConnectedImages(const ConnectedImages&) = delete;
	ConnectedImages& operator=(const ConnectedImages&) = delete;
	struct Range {
		Vec2D min, max;
		Range() {}
		Range(const Vec2D& a, const Vec2D& b): min(a), max(b) {}
		Vec2D size() const { return max - min; }
	};
	enum ProjectionMethod { flat, cylindrical, spherical };
	ProjectionMethod proj_method = flat;
	Range proj_range;
	int identity_idx = 0;
	struct ImageComponent {
		Homography homo, homo_inv;
		ImageRef* imgptr = nullptr;
		Range range;
		ImageComponent() {}
		ImageComponent(ImageRef* img): imgptr(img) {}
	};
	std::vector<ImageComponent> component;
	// Optional: the components' images, in component order, resident on the device (HipFeatureSet::views; not owned).  The
	// blend and the overlap passes then read view i for component i instead of uploading imgptr->img (hip_blend_images).
	const op_views* views = nullptr;
	// stitcher_image.cc:36-77: homo_inv from homo; ranges / proj_range / resolution from homo.  Kept
	// separate like the reference's: Stitcher::estimate_camera sets homo_inv = K R itself and only
	// calls update_proj_range() (stitcher.cc:154-158, :59)
	void calc_inverse_homo() { prepare(true, false); }
	void update_proj_range() { prepare(false, true); }
	Vec2D get_final_resolution() const { return resolution; }
	Mat32f blend() const;
	Vec2D resolution;
	private:
	void prepare(bool set_inverse, bool set_range);       // one host call of the C-ABI's geometry helper
};
#endif

// Geometry of a bundle through the C-ABI's host helper; fills homo_inv / range / proj_range the
// way ConnectedImages::calc_inverse_homo / update_proj_range do (stitcher_image.cc:36-77)
template <typename Bundle>
inline op_blend_geom hip_blend_prepare(const Bundle& b, std::vector<double>& hinv, std::vector<double>& ranges) {
	const int n = (int)b.component.size();
	std::vector<double> homo((size_t)n * 9); std::vector<int> shapes((size_t)n * 2);
	for (int i = 0; i < n; ++i) {
		for (int k = 0; k < 9; ++k) homo[(size_t)i * 9 + k] = b.component[i].homo[k];
		shapes[2 * i] = b.component[i].imgptr->width(); shapes[2 * i + 1] = b.component[i].imgptr->height();
	}
	hinv.assign((size_t)n * 9, 0); ranges.assign((size_t)n * 4, 0);
	op_blend_geom g;
	const op_config cfg = hip_config_snapshot();
	PANO_HIP_CHECK(op_blend_prepare(&cfg, (int)b.proj_method, b.identity_idx, n, shapes.data(), homo.data(), &g, hinv.data(), ranges.data()));
	return g;
}

// ConnectedImages::blend() (stitch/stitcher_image.cc:116-155) on the device.  Uses the bundle's
// own homo_inv / range / proj_range (already filled by calc_inverse_homo / update_proj_range)
// and the resolution of get_final_resolution(); the blender is chosen like the reference does
// (config::MULTIBAND > 0 ? MultiBandBlender : LinearBlender).
// crop = true additionally applies crop() (lib/imgproc.cc:200-235; main.cc:226-229 under config
// CROP) on the device, so only the cropped pixels cross PCIe.
// Exposure (gain) compensation -- an extension beyond the reference (Brown & Lowe, IJCV 2007, section 6; the C-ABI's
// op_gain_overlap + op_gain_solve): the n x 3 gains that equalise the bundle's overlaps, from the samples the linear
// blender takes on the canvas lattice of the given stride.  Pass them to hip_blend(b, crop, gains).
// the bundle's resident views, when it has the member (the reference's ConnectedImages has none)
template <typename Bundle> inline auto hip_bundle_views(const Bundle& b, int) -> decltype(b.views) { return b.views; }
template <typename Bundle> inline const op_views* hip_bundle_views(const Bundle&, long) { return nullptr; }
// the bundle's projection, range and resolution as the C-ABI's op_blend_geom; a component's homo_inv and range into its op_blend_image
template <typename Bundle>
inline void hip_bundle_geom(const Bundle& b, op_blend_geom& g) {
	const Vec2D res = b.get_final_resolution();
	g.proj_method = (int)b.proj_method;
	g.proj_min[0] = b.proj_range.min.x; g.proj_min[1] = b.proj_range.min.y;
	g.proj_max[0] = b.proj_range.max.x; g.proj_max[1] = b.proj_range.max.y;
	g.resolution[0] = res.x; g.resolution[1] = res.y;
}
template <typename Component>
inline void hip_component_geom(const Component& c, op_blend_image& im) {
	for (int k = 0; k < 9; ++k) im.homo_inv[k] = c.homo_inv[k];
	im.range[0] = c.range.min.x; im.range[1] = c.range.min.y; im.range[2] = c.range.max.x; im.range[3] = c.range.max.y;
}
template <typename Bundle>
inline std::vector<op_blend_image> hip_blend_images(const Bundle& b, op_blend_geom& g) {
	const int n = (int)b.component.size();
	hip_bundle_geom(b, g);
	std::vector<op_blend_image> ims(n);
	const op_views* views = hip_bundle_views(b, 0);
	if (views && op_views_count(views) != n) { fprintf(stderr, "hip_blend_images: %d resident views for %d components\n", op_views_count(views), n); exit(1); }
	for (int i = 0; i < n; ++i) {
		auto& c = b.component[i];
		c.imgptr->load();
		ims[i].h = c.imgptr->height(); ims[i].w = c.imgptr->width(); ims[i].on_device = 0;
		if (c.imgptr->img) {
			ims[i].data = c.imgptr->img->ptr();
			ims[i].mat_h = c.imgptr->img->height(); ims[i].mat_w = c.imgptr->img->width();      // != h / w after a cylinder pre-warp (op_blend_image)
		} else {    // decoded on the device (HipStitcher::jpeg_paths): the resident view is the only copy
			ims[i].data = nullptr; ims[i].mat_h = ims[i].h; ims[i].mat_w = ims[i].w;
			if (!views) { fprintf(stderr, "hip_blend_images: component %d has neither host pixels nor a resident view\n", i); exit(1); }
		}
		if (views) {    // the resident view stands for the Mat it was uploaded from; a Mat replaced since (cylinder pre-warp) keeps the host path
			op_blend_image v;
			PANO_HIP_CHECK(op_views_blend_image(views, i, &v));
			if (v.h == ims[i].mat_h && v.w == ims[i].mat_w && ims[i].mat_h == ims[i].h && ims[i].mat_w == ims[i].w) {
				ims[i].data = v.data; ims[i].on_device = v.on_device;
			}
		}
		if (!ims[i].data) { fprintf(stderr, "hip_blend_images: resident view %d is %d x %d, its component %d x %d\n", i, ims[i].mat_w, ims[i].mat_h, ims[i].w, ims[i].h); exit(1); }
		hip_component_geom(c, ims[i]);
	}
	return ims;
}
template <typename Bundle>
inline std::vector<float> hip_gain_compensate(const Bundle& b, int stride = 1, double sigma_n = 10.0 / 255.0, double sigma_g = 0.1,
		bool per_channel = true) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	const int n = (int)b.component.size();
	op_blend_geom g;
	const std::vector<op_blend_image> ims = hip_blend_images(b, g);
	const size_t npairs = (size_t)n * (n - 1) / 2;
	std::vector<int64_t> count(npairs + 1), sums(6 * npairs + 1);
	std::vector<float> gains((size_t)3 * n);
	PANO_HIP_CHECK(op_gain_overlap(ctx, &cfg, &g, ims.data(), n, stride, count.data(), sums.data()));
	PANO_HIP_CHECK(op_gain_solve(n, count.data(), sums.data(), sigma_n, sigma_g, per_channel ? 1 : 0, gains.data()));
	return gains;
}
// Block gain compensation (the C-ABI's op_gain_block_overlap + op_gain_block_solve): one gain per block of a bx x by grid
// on every image, which also evens out vignetting and brightness gradients inside a view.  Returns n * by * bx * 3 gains,
// [((k * by + v) * bx + u) * 3 + c]; pass them to hip_blend(b, crop, gains, bx, by).
template <typename Bundle>
inline std::vector<float> hip_gain_compensate_blocks(const Bundle& b, int bx, int by, int stride = 1, double sigma_n = 10.0 / 255.0,
		double sigma_g = 0.1, double sigma_s = 0.1, bool per_channel = true) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	const int n = (int)b.component.size();
	op_blend_geom g;
	const std::vector<op_blend_image> ims = hip_blend_images(b, g);
	const size_t B = (size_t)bx * by, entries = (size_t)n * (n - 1) / 2 * B * B;
	std::vector<int64_t> count(entries + 1), sums(6 * entries + 1);
	std::vector<float> gains(3 * (size_t)n * B);
	PANO_HIP_CHECK(op_gain_block_overlap(ctx, &cfg, &g, ims.data(), n, stride, bx, by, count.data(), sums.data()));
	PANO_HIP_CHECK(op_gain_block_solve(n, bx, by, count.data(), sums.data(), sigma_n, sigma_g, sigma_s, per_channel ? 1 : 0, gains.data()));
	return gains;
}

// Vignetting compensation (the C-ABI's op_vignette_overlap + op_vignette_solve): n x 3 grey exposure gains (returned) and
// one radial falloff curve V(rho) = 1 + a1 rho + a2 rho^2 + a3 rho^3 shared by all views (poly = a1, a2, a3); pass both to
// hip_blend(b, crop, gains, poly).  When the fitted curve is not positive on [0, 1] (the solve's OP_ERR_UNSUPPORTED) this
// keeps plain gains: hip_gain_compensate's, with poly = 0.
template <typename Bundle>
inline std::vector<float> hip_vignette_compensate(const Bundle& b, std::array<float, 3>& poly, int stride = 2, float clip = 0.98f,
		int degree = 3, double sigma_n = 10.0 / 255.0, double sigma_g = 1.0, double sigma_v = 100.0) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	const int n = (int)b.component.size();
	op_blend_geom g;
	const std::vector<op_blend_image> ims = hip_blend_images(b, g);
	const size_t npairs = (size_t)n * (n - 1) / 2;
	std::vector<int64_t> count(npairs + 1), moments(30 * npairs + 1);
	std::vector<float> gains((size_t)3 * n);
	PANO_HIP_CHECK(op_vignette_overlap(ctx, &cfg, &g, ims.data(), n, stride, clip, count.data(), moments.data()));
	const int rc = op_vignette_solve(n, count.data(), moments.data(), degree, sigma_n, sigma_g, sigma_v, gains.data(), poly.data());
	if (rc == OP_ERR_UNSUPPORTED) {
		fprintf(stderr, "hip_vignette_compensate: %s\n", op_last_error());
		poly = {0.f, 0.f, 0.f};
		return hip_gain_compensate(b);
	}
	PANO_HIP_CHECK(rc);
	return gains;
}

// gains: empty = op_blend; bx = by = 0: n x 3 exposure gains (op_blend_gains); bx, by >= 1: n x by x bx x 3 block gains
// (op_blend_block_gains)
// the blend as the device canvas the caller owns (op_canvas_free): for the crop, the encoders and hip_reproject in place
template <typename Bundle>
inline op_canvas* hip_blend_canvas(const Bundle& b, const std::vector<float>& gains, int bx, int by, const float* poly = nullptr) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	const int n = (int)b.component.size();
	op_blend_geom g;
#ifdef OPENPANO_WITH_REFERENCE
	{	// the line ConnectedImages::blend prints (stitcher_image.cc:121-124); the reference's run_test.py scrapes it
		const Vec2D size_d = b.proj_range.size() / b.get_final_resolution();
		const Coor size(size_d.x, size_d.y);
		print_debug("Final Image Size: (%d, %d)\n", size.x, size.y);
	}
#endif
	const std::vector<op_blend_image> ims = hip_blend_images(b, g);
	const size_t per_image = bx > 0 ? (size_t)3 * bx * by : 3;
	if (!gains.empty() && gains.size() != per_image * n) { fprintf(stderr, "hip_blend: %zu gains for %d images\n", gains.size(), n); exit(1); }
	HipCanvas cv;
	if (poly) PANO_HIP_CHECK(op_blend_vignette(ctx, &cfg, &g, ims.data(), n, gains.empty() ? nullptr : gains.data(), poly, hip_out(cv)));
	else if (gains.empty()) PANO_HIP_CHECK(op_blend(ctx, &cfg, &g, ims.data(), n, hip_out(cv)));
	else if (bx > 0) PANO_HIP_CHECK(op_blend_block_gains(ctx, &cfg, &g, ims.data(), n, bx, by, gains.data(), hip_out(cv)));
	else PANO_HIP_CHECK(op_blend_gains(ctx, &cfg, &g, ims.data(), n, gains.data(), hip_out(cv)));
	return cv.release();
}
template <typename Bundle>
inline Mat32f hip_blend(const Bundle& b, bool crop, const std::vector<float>& gains, int bx, int by, const float* poly = nullptr) {
	HipCanvas cv(hip_blend_canvas(b, gains, bx, by, poly));
	if (crop) hip_crop_in_place(cv);
	return hip_canvas_to_mat(std::move(cv));
}

// gains: empty = op_blend, else n x 3 exposure gains (op_blend_gains)
template <typename Bundle>
inline Mat32f hip_blend(const Bundle& b, bool crop, const std::vector<float>& gains) { return hip_blend(b, crop, gains, 0, 0); }
// gains: n x 3 grey exposure gains (empty = 1) under the shared vignetting curve poly = a1, a2, a3 (op_blend_vignette)
template <typename Bundle>
inline Mat32f hip_blend(const Bundle& b, bool crop, const std::vector<float>& gains, const std::array<float, 3>& poly) {
	return hip_blend(b, crop, gains, 0, 0, poly.data());
}
template <typename Bundle>
inline Mat32f hip_blend(const Bundle& b, bool crop = false) { return hip_blend(b, crop, std::vector<float>()); }

// The photometric compensation a job asks for, then the blend that applies it -- both after the bundle's geometry is final.
// gain: exposure gains (hip_gain_compensate), one per block of a bx x by grid on every image when bx * by > 1
// (hip_gain_compensate_blocks); vignetting: grey gains plus the shared falloff curve (hip_vignette_compensate), refused
// together with block gains.  `gains` and `vignette_poly` receive what the blend used (empty / 0 when it used none).
struct HipCompensation {
	bool gain = false;
	int bx = 1, by = 1;
	bool vignetting = false;
};
template <typename Bundle>
inline op_canvas* hip_compensate_and_blend_canvas(const Bundle& b, const HipCompensation& how, std::vector<float>& gains, std::array<float, 3>& vignette_poly) {
	vignette_poly = {0.f, 0.f, 0.f};
	if (how.vignetting) {
		if (how.bx * how.by > 1) { fprintf(stderr, "HipStitcher: vignetting and block gains are exclusive\n"); exit(1); }
		gains = hip_vignette_compensate(b, vignette_poly);
		return hip_blend_canvas(b, gains, 0, 0, vignette_poly.data());
	}
	if (!how.gain) { gains.clear(); return hip_blend_canvas(b, gains, 0, 0); }
	if (how.bx == 1 && how.by == 1) {
		gains = hip_gain_compensate(b);
		return hip_blend_canvas(b, gains, 0, 0);
	}
	gains = hip_gain_compensate_blocks(b, how.bx, how.by);
	return hip_blend_canvas(b, gains, how.bx, how.by);
}
template <typename Bundle>
inline Mat32f hip_compensate_and_blend(const Bundle& b, const HipCompensation& how, std::vector<float>& gains, std::array<float, 3>& vignette_poly) {
	return hip_canvas_to_mat(HipCanvas(hip_compensate_and_blend_canvas(b, how, gains, vignette_poly)));
}

// ---- a finished equirectangular panorama looked at again (op_canvas_reproject): planet (main.cc:294-331), a rectilinear view,
// the faces of a cube.  The canvas stays on the device; the result is a canvas the caller owns, ready for the encoders.
// hip_pano_frame: where the canvas of a spherical bundle sits on the sphere, or its crop at (x0, y0); wrap is the caller's statement
// that the columns span exactly one turn.
template <typename Bundle>
inline op_pano_frame hip_pano_frame(const Bundle& b, int x0 = 0, int y0 = 0, bool wrap = false) {
	op_blend_geom g;
	hip_bundle_geom(b, g);
	op_pano_frame f;
	PANO_HIP_CHECK(op_pano_frame_of(&g, x0, y0, &f));
	f.wrap = wrap ? 1 : 0;
	return f;
}
inline op_canvas* hip_reproject(const op_canvas* canvas, const op_pano_frame& frame, const op_view_spec& spec) {
	op_canvas* out = nullptr;
	PANO_HIP_CHECK(op_canvas_reproject(HipContext::get(), canvas, &frame, &spec, &out));
	return out;
}
inline op_view_spec hip_view_look(double yaw, double pitch, double roll, double hfov, int out_w, int out_h) {
	op_view_spec s;
	PANO_HIP_CHECK(op_view_look(yaw, pitch, roll, hfov, out_w, out_h, &s));
	return s;
}
inline op_view_spec hip_view_cube_face(int face, int n) {
	op_view_spec s;
	PANO_HIP_CHECK(op_view_cube_face(face, n, &s));
	return s;
}
inline op_view_spec hip_view_planet(int n) {
	op_view_spec s;
	PANO_HIP_CHECK(op_view_planet(n, &s));
	return s;
}

// ---- write_rgb(fname, mat) (lib/imgio.cc:25-41,98-113; main.cc:30,226-233): the file is encoded on the device instead of on one
// host thread.  What both formats share: the bytes of the handle an encoder returned go into fname and the handle is freed
// (size / copy: the format's C entries; its free is the handle's own), and a host matrix is quantised as write_rgb does it (Color::NO ->
// white, v * 255 truncated).
template <typename File, void (*Free)(File*)>
inline void hip_write_encoded(const char* fname, HipHandle<File, Free> file, int64_t (*size)(const File*), int (*copy)(op_ctx*, const File*, unsigned char*),
		const char* who) {
	std::vector<unsigned char> bytes((size_t)size(file.get()));
	if (copy(HipContext::get(), file.get(), bytes.data()) != OP_OK) hip_error_exit(who);
	file.reset();
	FILE* f = fopen(fname, "wb");
	if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) {
		fprintf(stderr, "%s: cannot write %s\n", who, fname);
		exit(1);
	}
}
inline std::vector<unsigned char> hip_quantise_rgb(const Mat32f& mat) {
	std::vector<unsigned char> rgb((size_t)mat.rows() * mat.cols() * 3);
	const float* p = mat.ptr();
	for (size_t i = 0; i < rgb.size(); ++i) rgb[i] = (unsigned char)((p[i] < 0 ? 1 : p[i]) * 255);
	return rgb;
}

// ---- a .png name: op_canvas_encode_png / op_png_encode_u8 stand in for lodepng.  Same pixels as the reference's file, 8-bit RGB
// where lodepng is handed RGBA with alpha 255 and reduces it to RGB.
inline void hip_write_png_file(const char* fname, HipPng png) { hip_write_encoded(fname, std::move(png), op_png_size, op_png_copy, "hip_write_png"); }
// the device canvas a blend left behind (op_blend*, op_canvas_crop): the fp32 canvas does not come back at all
inline void hip_write_png(const char* fname, const op_canvas* canvas) {
	HipPng png;
	PANO_HIP_CHECK(op_canvas_encode_png(HipContext::get(), canvas, hip_out(png)));
	hip_write_png_file(fname, std::move(png));
}
// write_rgb's signature: a matrix in host memory
inline void hip_write_png(const char* fname, const Mat32f& mat) {
	const std::vector<unsigned char> rgb = hip_quantise_rgb(mat);
	HipPng png;
	PANO_HIP_CHECK(op_png_encode_u8(HipContext::get(), rgb.data(), mat.rows(), mat.cols(), hip_out(png)));
	hip_write_png_file(fname, std::move(png));
}

// ---- a .jpg name (-> CImg::save_jpeg -> libjpeg): baseline JPEG from op_canvas_encode_jpeg / op_jpeg_encode_u8, every byte what
// libjpeg writes for the same pixels, quality, sampling and restart interval.  The reference's own file is quality 100 at OP_JPEG_420.
inline void hip_write_jpeg_file(const char* fname, HipJpeg jpg) { hip_write_encoded(fname, std::move(jpg), op_jpeg_size, op_jpeg_copy, "hip_write_jpeg"); }
// the device canvas a blend left behind (op_blend*, op_canvas_crop)
inline void hip_write_jpeg(const char* fname, const op_canvas* canvas, int quality = 90, int subsampling = OP_JPEG_420) {
	HipJpeg jpg;
	PANO_HIP_CHECK(op_canvas_encode_jpeg(HipContext::get(), canvas, quality, subsampling, hip_out(jpg)));
	hip_write_jpeg_file(fname, std::move(jpg));
}
// write_rgb's signature: a matrix in host memory
inline void hip_write_jpeg(const char* fname, const Mat32f& pano, int quality = 90, int subsampling = OP_JPEG_420) {
	const std::vector<unsigned char> rgb = hip_quantise_rgb(pano);
	HipJpeg jpg;
	PANO_HIP_CHECK(op_jpeg_encode_u8(HipContext::get(), rgb.data(), pano.rows(), pano.cols(), quality, subsampling, hip_out(jpg)));
	hip_write_jpeg_file(fname, std::move(jpg));
}

#ifndef OPENPANO_WITH_REFERENCE
inline void ConnectedImages::prepare(bool set_inverse, bool set_range) {
	std::vector<double> hinv, ranges;
	const op_blend_geom g = hip_blend_prepare(*this, hinv, ranges);
	for (size_t i = 0; i < component.size(); ++i) {
		if (set_inverse) for (int k = 0; k < 9; ++k) component[i].homo_inv[k] = hinv[i * 9 + k];
		if (set_range) component[i].range = Range(Vec2D(ranges[4 * i], ranges[4 * i + 1]), Vec2D(ranges[4 * i + 2], ranges[4 * i + 3]));
	}
	if (set_range) {
		proj_range = Range(Vec2D(g.proj_min[0], g.proj_min[1]), Vec2D(g.proj_max[0], g.proj_max[1]));
		resolution = Vec2D(g.resolution[0], g.resolution[1]);
	}
}
inline Mat32f ConnectedImages::blend() const { return hip_blend(*this); }
#endif

#ifdef OPENPANO_WITH_REFERENCE
// Hook 6 (HOST-ONLY, optional): CameraEstimator{pairwise_matches, shapes}.estimate() of Stitcher::estimate_camera
// (stitch/stitcher.cc:143-146 -> camera_estimator.cc:46-103 -> incremental_bundle_adjuster.cc:117-385) through
// libpano_host.so, the Eigen-free estimator of host/pano_camera.hh: same constructor arguments, same estimate().  The
// reference's bundle adjuster materialises and zeroes a (2 x matches) x (6 x images) Jacobian per iteration
// (incremental_bundle_adjuster.cc:280); the mirror accumulates J^T J block by block in the reference's summation order --
// the cameras are the reference's, digit for digit (tests/test_camera_vs_ref.py; both sides then solve through the same
// QR / SVD arithmetic, i.e. parity is unpinned at Eigen's own rounding only).  Unlike the reference class this one does
// not write back into `matches` (camera_estimator.hh:33); Stitcher::build() clears them right after (stitcher.cc:54).
class HostCameraEstimator {
	public:
		HostCameraEstimator(std::vector<std::vector<MatchInfo>>& matches, const std::vector<Shape2D>& image_shapes):
			matches(matches), shapes(image_shapes) {}
		std::vector<Camera> estimate() {
			GuardedTimer tm("Estimate Camera");                  // the reference's own label (camera_estimator.cc:47)
			pano_config_set("STRAIGHTEN", (float)config::STRAIGHTEN); pano_config_set("MULTIPASS_BA", (float)config::MULTIPASS_BA);
			pano_config_set("LM_LAMBDA", (float)config::LM_LAMBDA); pano_config_set("ESTIMATE_CAMERA", (float)config::ESTIMATE_CAMERA);
			pano_config_set("ORDERED_INPUT", (float)config::ORDERED_INPUT); pano_config_set("TRANS", (float)config::TRANS);
			pano_config_set("CYLINDER", (float)config::CYLINDER);
			const int n = (int)matches.size();
			std::vector<int> wh, ij, cnt; std::vector<float> conf; std::vector<double> homo, pts;
			for (auto& s : shapes) { wh.push_back(s.w); wh.push_back(s.h); }
			for (int i = 0; i < n; ++i)
				for (int j = 0; j < n; ++j) {
					const MatchInfo& m = matches[i][j];
					if (m.match.empty() && m.confidence == 0) continue;           // never assigned by match_image (stitcher.cc:79-93)
					ij.push_back(i); ij.push_back(j); conf.push_back(m.confidence); cnt.push_back((int)m.match.size());
					for (int k = 0; k < 9; ++k) homo.push_back(m.homo[k]);
					for (auto& p : m.match) { pts.push_back(p.first.x); pts.push_back(p.first.y); pts.push_back(p.second.x); pts.push_back(p.second.y); }
				}
			std::vector<double> out((size_t)n * 13);
			if (pts.empty()) pts.push_back(0);
			pano_estimate_cameras(n, wh.data(), (int)cnt.size(), ij.data(), conf.data(), homo.data(), cnt.data(), pts.data(), out.data());
			std::vector<Camera> cams(n);
			for (int i = 0; i < n; ++i) {
				const double* o = out.data() + 13 * (size_t)i;
				cams[i].focal = o[0]; cams[i].aspect = o[1]; cams[i].ppx = o[2]; cams[i].ppy = o[3];
				for (int k = 0; k < 9; ++k) cams[i].R[k] = o[4 + k];
			}
			return cams;
		}
	private:
		std::vector<std::vector<MatchInfo>>& matches;
		const std::vector<Shape2D>& shapes;
};
#endif

// CylinderWarper (stitch/warp.hh:42-61): same method set
class HipCylinderWarper {
	public:
		explicit HipCylinderWarper(double m_hfactor): h_factor(m_hfactor) {}
		// warp image together with key points
		void warp(Mat32f& mat, std::vector<Vec2D>& kpts) const {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			Shape2D shape(mat.width(), mat.height());
			op_image im{mat.ptr(), mat.rows(), mat.cols(), 0, OP_F32};
			HipCanvas cv;
			PANO_HIP_CHECK(op_cyl_warp(ctx, &cfg, &im, h_factor, hip_out(cv)));
			warp(shape, kpts);
			mat = hip_canvas_to_mat(std::move(cv));
		}
		// warp keypoints given image shape
		void warp(Shape2D& shape, std::vector<Vec2D>& kpts) const {
			const op_config cfg = hip_config_snapshot();
			std::vector<double> p = hip_flatten(kpts);
			int nw, nh; double off[2];
			PANO_HIP_CHECK(op_cyl_warp_shape(&cfg, shape.w, shape.h, h_factor, kpts.empty() ? nullptr : p.data(), (int)kpts.size(), &nw, &nh, off));
			hip_unflatten(p, kpts);
			shape.w = nw; shape.h = nh;
		}
		// warp image only
		void warp(Mat32f& mat) const { std::vector<Vec2D> a; warp(mat, a); }
	protected:
		const double h_factor;
};

// CylinderStitcher::perspective_correction (stitch/cylstitcher.cc:139-180) on the device: the corners of the bundle's first and
// last component in the blended canvas (op_perspective_homography, host fp64) and the LinearBlender pass that stretches them to
// the canvas rectangle (op_canvas_perspective) -- always the linear blender, as in the reference.  `canvas` is what the blend
// left on the device (op_blend*); the result is a new canvas the caller owns, ready for op_canvas_crop and the encoders.
// corners / inv (optional): the 4 x 2 corners and the 3 x 3 map, for callers that report them.  Hook 4 of INTEGRATION.md.
template <typename Bundle>
inline op_canvas* hip_perspective_correction(const Bundle& b, const op_canvas* canvas, double* corners = nullptr, double* inv = nullptr) {
	op_ctx* ctx = HipContext::get();
	const op_config cfg = hip_config_snapshot();
	int h, w;
	PANO_HIP_CHECK(op_canvas_dims(canvas, &h, &w));
	op_blend_geom g;
	memset(&g, 0, sizeof g);
	g.proj_min[0] = b.proj_range.min.x; g.proj_min[1] = b.proj_range.min.y;
	const auto& ref = *b.component[b.identity_idx].imgptr;
	const auto& first = b.component.front();
	const auto& last = b.component.back();
	double fh[9], lh[9], m[9];
	for (int k = 0; k < 9; ++k) { fh[k] = first.homo[k]; lh[k] = last.homo[k]; }
	PANO_HIP_CHECK(op_perspective_homography(&g, ref.width(), ref.height(), first.imgptr->width(), first.imgptr->height(), fh,
			last.imgptr->width(), last.imgptr->height(), lh, w, h, m, corners));
	if (inv) memcpy(inv, m, sizeof m);
	op_canvas* out = nullptr;
	PANO_HIP_CHECK(op_canvas_perspective(ctx, &cfg, canvas, m, &out));
	return out;
}
// perspective_correction's own signature: a matrix in host memory goes up, the corrected one comes back
template <typename Bundle>
inline Mat32f hip_perspective_correction(const Bundle& b, const Mat32f& img) {
	HipCanvas cv;
	PANO_HIP_CHECK(op_canvas_upload(HipContext::get(), img.ptr(), img.rows(), img.cols(), hip_out(cv)));
	HipCanvas fixed(hip_perspective_correction(b, cv.get()));
	cv.reset();
	return hip_canvas_to_mat(std::move(fixed));
}

#ifndef OPENPANO_WITH_REFERENCE
// ===================================== STITCHER BASE =====================================
// ImageRef(fname) for a list of baseline JPEG files (stitch/imageref.hh:15-31): only the headers are read (op_jpeg_probe), for the
// shapes; with apply_exif_orientation a file of orientation 5..8 enters as w x h.  For HipStitcherBase's file constructor.
inline void hip_jpeg_image_refs(const std::vector<std::string>& paths, bool apply_exif_orientation, std::vector<ImageRef>& imgs) {
	for (auto& p : paths) {
		std::vector<unsigned char> head = hip_read_file(p, 1 << 20);     // SOF0 comes before the scan; a megabyte holds any EXIF before it
		if (head.size() == (size_t)1 << 20) head = hip_read_file(p);     // a longer file is read whole
		int h = 0, w = 0, sampling = 0;
		if (op_jpeg_probe(head.data(), (int64_t)head.size(), &h, &w, &sampling) != OP_OK) hip_error_exit(p);
		if (apply_exif_orientation) {
			int o = 1;
			if (op_jpeg_exif(head.data(), (int64_t)head.size(), &o, nullptr) != OP_OK) hip_error_exit(p);
			if (o >= 5) std::swap(h, w);
		}
		imgs.emplace_back(p);
		imgs.back()._width = w; imgs.back()._height = h;
	}
}

// What the two stitchers share (the part StitcherBase has in the reference): the image list from matrices or from camera files,
// the features and keypoints of all images from one batched call, and the bundle whose components point at the images.
class HipStitcherBase {
	public:
		HipStitcherBase(const HipStitcherBase&) = delete;
		HipStitcherBase& operator=(const HipStitcherBase&) = delete;

		std::vector<ImageRef> imgs;
		HipFeatureSet feats;                                        // StitcherBase::feats + the resident device copy
		std::vector<std::vector<Vec2D>> keypoints;
		ConnectedImages bundle;
		uint32_t base_seed;
		// resident views: calc_feature uploads the images once (bytes when they are exact k / 255, fp32 otherwise) and every
		// later stage reads that upload -- SIFT, and then the overlap passes and the blend (HipStitcher) or the cylinder
		// pre-warp (HipCylinderStitcher); off by default.  The panorama is the same bit for bit.
		bool resident_views = false;
		// with jpeg_paths: calc_feature() decodes every view turned upright by its file's EXIF orientation
		// (hip_read_jpeg_views(.., true)); off by default, as the reference ignores the tag.  Set through the constructor,
		// which takes the shapes of the views
		bool apply_exif_orientation = false;
		// set by the constructor that takes files: the views are decoded on the device and always resident
		std::vector<std::string> jpeg_paths;

		std::vector<Shape2D> shapes() const {
			std::vector<Shape2D> s;
			for (auto& r : imgs) s.push_back(r.shape());
			return s;
		}
		void calc_feature() {                                       // stitcherbase.cc:9-27
			std::vector<const Mat32f*> ptrs;
			for (auto& r : imgs) ptrs.push_back(r.img);
			bundle.views = nullptr;                                 // the previous upload is released by the assignment below
			if (!jpeg_paths.empty()) feats = HipSIFTDetector().calc_feature(hip_read_jpeg_views(HipContext::get(), jpeg_paths, apply_exif_orientation));
			else feats = HipSIFTDetector().calc_feature(ptrs, resident_views);
			keypoints.clear();
			for (auto& f : feats.feats) keypoints.push_back(hip_keypoints(f));
		}
		void free_feature() { feats = HipFeatureSet(); keypoints.clear(); }     // stitcherbase.cc:29-33; the views go with it

	protected:
		HipStitcherBase(const std::vector<Mat32f>& mats, uint32_t base_seed, bool resident_views): HipStitcherBase(mats.size(), base_seed) {
			this->resident_views = resident_views;
			for (auto& m : mats) imgs.emplace_back(m);
			for (auto& r : imgs) bundle.component.emplace_back(&r);
		}
		// From camera files: jpeg_paths stands in place of the Mat32f images (ImageRef(fname), stitch/imageref.hh:15-31).  Only
		// the headers are read here (op_jpeg_probe, for the shapes); calc_feature() decodes the files on the device
		// (hip_read_jpeg_views) and every later stage reads those views: a build touches no host pixel.
		// apply_exif_orientation: the views are turned upright by their files' EXIF orientation, so a file of orientation
		// 5..8 enters the job as w x h.
		HipStitcherBase(const std::vector<std::string>& paths, uint32_t base_seed, bool apply_exif_orientation): HipStitcherBase(paths.size(), base_seed) {
			this->apply_exif_orientation = apply_exif_orientation;
			jpeg_paths = paths;
			hip_jpeg_image_refs(paths, apply_exif_orientation, imgs);
			for (auto& r : imgs) bundle.component.emplace_back(&r);
		}
		~HipStitcherBase() = default;
	private:
		HipStitcherBase(size_t n, uint32_t base_seed): base_seed(base_seed) {
			if (n <= 1) { fprintf(stderr, "Cannot stitch with only %zu images.\n", n); exit(1); }   // stitcherbase.hh:46-48
		}
};

// ===================================== STITCHER =====================================
// Stitcher (stitch/stitcher.hh:17-62, stitcher.cc:32-198), standalone: the whole of Stitcher::build() with the device stages
// batched -- one SIFT call for all images, one match call and one RANSAC call for the whole pair list -- and the host stages
// (camera estimation / bundle adjustment, pano_camera.hh) in between.  Members keep the reference's names; `cameras` and
// `base_seed` (RANSAC seed injection) are additions.
class HipStitcher : public HipStitcherBase {
	public:
		explicit HipStitcher(const std::vector<Mat32f>& mats, uint32_t base_seed = 42u): HipStitcherBase(mats, base_seed, false) {}
		explicit HipStitcher(const std::vector<std::string>& paths, uint32_t base_seed = 42u, bool apply_exif_orientation = false):
				HipStitcherBase(paths, base_seed, apply_exif_orientation) {}

		Mat32f build() {                                            // stitcher.cc:32-64
			prepare_blend();
			const HipCompensation how{gain_compensation, gain_blocks_x, gain_blocks_y, vignetting};
			return hip_compensate_and_blend(bundle, how, gains, vignette_poly);   // after the homographies are final
		}
		void prepare_blend() {                                      // build() up to the blend
			calc_feature();
			bundle.views = resident_views || !jpeg_paths.empty() ? feats.views.get() : nullptr;
			pairwise_matches.assign(imgs.size(), std::vector<MatchInfo>(imgs.size()));
			if (config::ORDERED_INPUT) linear_pairwise_match();
			else pairwise_match();
			assign_center();
			if (config::ESTIMATE_CAMERA) estimate_camera();
			else build_linear_simple();
			bundle.proj_method = config::ESTIMATE_CAMERA ? ConnectedImages::spherical : ConnectedImages::flat;
			bundle.update_proj_range();
		}

		// build() with the panorama left on the device (the caller owns the canvas: op_canvas_free), cropped to its largest valid
		// rectangle under `crop`; hip_write_png / hip_write_jpeg and hip_reproject take it in place
		op_canvas* build_canvas(bool crop = false) {
			prepare_blend();
			const HipCompensation how{gain_compensation, gain_blocks_x, gain_blocks_y, vignetting};
			HipCanvas cv(hip_compensate_and_blend_canvas(bundle, how, gains, vignette_poly));
			crop_x0 = crop_y0 = 0;
			if (crop) {
				HipCanvas cropped;
				PANO_HIP_CHECK(op_canvas_crop(HipContext::get(), cv.get(), hip_out(cropped), &crop_x0, &crop_y0));
				cv = std::move(cropped);
			}
			return cv.release();
		}
		// where the canvas of the last build_canvas() sits on the sphere (ESTIMATE_CAMERA builds only), its crop origin included
		int crop_x0 = 0, crop_y0 = 0;
		op_pano_frame pano_frame(bool wrap = false) const { return hip_pano_frame(bundle, crop_x0, crop_y0, wrap); }

		std::vector<std::vector<MatchInfo>> pairwise_matches;
		std::vector<Camera> cameras;
		// exposure (gain) compensation before the blend (hip_gain_compensate): an extension, off by default; `gains` holds
		// the n x 3 gains the last build() used (empty when it used none).  gain_blocks_x / _y > 1: one gain per block of
		// that grid on every image (hip_gain_compensate_blocks); `gains` then holds n * by * bx * 3
		bool gain_compensation = false;
		int gain_blocks_x = 1, gain_blocks_y = 1;
		// vignetting: grey gains plus one radial falloff curve shared by all views (hip_vignette_compensate), off by default,
		// refused together with block gains; `gains` then holds n x 3 and vignette_poly the curve's a1..a3 (0 otherwise)
		bool vignetting = false;
		std::array<float, 3> vignette_poly = {0.f, 0.f, 0.f};
		std::vector<float> gains;

		void pairwise_match() { match_tasks(hip_default_tasks((int)imgs.size(), false), false); }          // stitcher.cc:96-113
		void linear_pairwise_match() { match_tasks(hip_default_tasks((int)imgs.size(), true), true); }      // stitcher.cc:115-136
		void assign_center() { bundle.identity_idx = (int)imgs.size() >> 1; }   // stitcher.cc:138-141
		void estimate_camera() {                                    // stitcher.cc:143-158
			cameras = CameraEstimator{pairwise_matches, shapes()}.estimate();
			for (size_t i = 0; i < imgs.size(); ++i) {
				bundle.component[i].homo_inv = cameras[i].K() * cameras[i].R;
				bundle.component[i].homo = cameras[i].Rinv() * cameras[i].K().inverse();
			}
		}
		void build_linear_simple() {                                // stitcher.cc:160-198
			const int n = (int)imgs.size(), mid = bundle.identity_idx;
			auto& comp = bundle.component;
			comp[mid].homo = Homography::I();
			if (mid + 1 < n) {
				comp[mid + 1].homo = pairwise_matches[mid][mid + 1].homo;
				for (int k = mid + 2; k < n; ++k) comp[k].homo = comp[k - 1].homo * pairwise_matches[k - 1][k].homo;
			}
			if (mid - 1 >= 0) {
				comp[mid - 1].homo = pairwise_matches[mid][mid - 1].homo;
				for (int k = mid - 2; k >= 0; --k) comp[k].homo = comp[k + 1].homo * pairwise_matches[k + 1][k].homo;
			}
			double f = -1;
			if (!config::TRANS) f = Camera::estimate_focal(pairwise_matches);
			if (f <= 0) f = 0.5 * (imgs[mid].width() + imgs[mid].height());
			for (int i = 0; i < n; ++i) {
				const double t[9] = {1.0 / f, 0, 0, 0, 1.0 / f, 0, 0, 0, 1};
				comp[i].homo = Homography(t) * comp[i].homo;
			}
			bundle.calc_inverse_homo();
		}

		// match_image (stitcher.cc:66-94) for a whole task list: one match call + one RANSAC call,
		// then the reference's bookkeeping per connected pair
		void match_tasks(const std::vector<std::pair<int, int>>& tasks, bool linear) {
			record_matches(tasks, hip_match_images(feats, shapes(), tasks, base_seed), linear);
		}
		void record_matches(const std::vector<std::pair<int, int>>& tasks, const std::vector<std::pair<bool, MatchInfo>>& infos, bool linear) {
			const int n = (int)imgs.size();
			for (size_t k = 0; k < tasks.size(); ++k) {
				const int i = tasks[k].first, j = tasks[k].second;
				if (!infos[k].first) {
					if (linear && i != n - 1) {       // head and tail don't have to match (stitcher.cc:123-127)
						fprintf(stderr, "error: Image %d and %d don't match\n", i, j);
						exit(1);
					}
					continue;
				}
				MatchInfo info = infos[k].second;
				Homography inv = info.homo.inverse();       // TransformEstimation ensures invertible
				inv.mult(1.0 / inv[8]);
				pairwise_matches[i][j] = info;
				info.homo = inv;
				info.reverse();
				pairwise_matches[j][i] = std::move(info);
			}
		}
};

// ===================================== CYLINDER STITCHER =====================================
// CylinderStitcher (stitch/cylstitcher.hh, cylstitcher.cc:20-180) + StitcherBase, standalone: the reference's mode for an ordered
// sweep at a known focal length (config CYLINDER).  Every pixel stage runs on the device and the pixels stay there: SIFT on the
// views, the cylinder pre-warp into device canvases (op_cyl_warp), the blend from those canvases (OP_SRC_DEVICE, h / w the
// ImageRef's stale size and mat_h / mat_w the warp's), the perspective correction (hip_perspective_correction) and, for
// build_canvas(true), the crop -- so that hip_write_png / hip_write_jpeg encode the result in place.  The h-factor search is the
// reference's, float for float; its RANSAC calls are batched: one op_match_pairs for the n - 1 neighbour pairs, one
// op_ransac_pairs per update_h_factor attempt over all right-hand pairs, one for all left-hand pairs, each over coordinates-only
// features (the warped keypoints).  Every estimate of one build() is seeded with base_seed (the reference seeds each from
// std::random_device).  Members keep the reference's names; `attempts`, `best_factor`, `corners`, `inv` record what a build did.
class HipCylinderStitcher : public HipStitcherBase {
	public:
		explicit HipCylinderStitcher(const std::vector<Mat32f>& mats, uint32_t base_seed = 42u, bool resident_views = false):
				HipStitcherBase(mats, base_seed, resident_views) {}
		// From camera files, as HipStitcher(paths): the views are decoded on the device and are always resident
		explicit HipCylinderStitcher(const std::vector<std::string>& paths, uint32_t base_seed = 42u, bool apply_exif_orientation = false):
				HipStitcherBase(paths, base_seed, apply_exif_orientation) {}
		~HipCylinderStitcher() { free_warped(); }

		// CylinderStitcher::build() (cylstitcher.cc:20-29) with the panorama left on the device; the caller owns it (op_canvas_free).
		// crop: crop() of main.cc:226-229 on the device as well
		op_canvas* build_canvas(bool crop = false) {
			calc_feature();
			bundle.identity_idx = (int)imgs.size() >> 1;
			build_warp();
			free_feature();
			bundle.proj_method = ConnectedImages::flat;
			bundle.update_proj_range();
			HipCanvas ret(blend());
			HipCanvas fixed(perspective_correction(ret.get()));
			ret.reset();
			if (crop) hip_crop_in_place(fixed);
			return fixed.release();
		}
		Mat32f build() { return hip_canvas_to_mat(HipCanvas(build_canvas())); }

		// what the last build did: every update_h_factor attempt, the factor the pre-warp used, the four corners and the map of
		// the perspective correction
		struct Attempt { float factor, slope; bool ok; };
		std::vector<Attempt> attempts;
		float best_factor = 1;
		double corners[8] = {0}, inv[9] = {0};
		// the pre-warped views, on the device (what imgs[k].img becomes in the reference, cylstitcher.cc:66-67)
		std::vector<op_canvas*> warped;

		void build_warp() {                                         // cylstitcher.cc:31-87
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			const int n = (int)imgs.size(), mid = bundle.identity_idx;
			for (int i = 0; i < n; ++i) bundle.component[i].homo = Homography::I();
			attempts.clear();

			// matches[k]: k, k + 1 (:41-42), once; the right-hand lists as they are and the left-hand ones reversed (:73) become
			// the two handles the RANSAC calls read
			std::vector<int> pr;
			for (int k = 0; k + 1 < n; ++k) { pr.push_back(k); pr.push_back(k + 1); }
			HipMatches all;
			PANO_HIP_CHECK(op_match_pairs(ctx, &cfg, feats.handle.get(), pr.data(), n - 1, hip_out(all)));
			std::vector<int64_t> off((size_t)n);
			std::vector<int> idx((size_t)op_matches_total(all.get()) * 2 + 2);
			PANO_HIP_CHECK(op_matches_copy_all(all.get(), idx.data(), off.data()));
			all.reset();
			for (int k = 0; k < mid; ++k) for (int64_t q = off[k]; q < off[k + 1]; ++q) std::swap(idx[2 * q], idx[2 * q + 1]);
			std::vector<const int*> lists; std::vector<int> counts;
			for (int k = 0; k + 1 < n; ++k) { lists.push_back(idx.data() + 2 * off[k]); counts.push_back((int)(off[k + 1] - off[k])); }
			if (n - 1 - mid > 0) PANO_HIP_CHECK(op_matches_from_host(lists.data() + mid, counts.data() + mid, n - 1 - mid, hip_out(right_matches)));
			if (mid > 0) PANO_HIP_CHECK(op_matches_from_host(lists.data(), counts.data(), mid, hip_out(left_matches)));

			std::vector<Homography> bestmat;
			float minslope = std::numeric_limits<float>::max();
			float bestfactor = 1;
			if (n - mid > 1) {
				float newfactor = 1;
				float slope = update_h_factor(newfactor, minslope, bestfactor, bestmat);
				if (bestmat.empty()) { fprintf(stderr, "error: Failed to find hfactor\n"); exit(1); }
				float centerx1 = 0, centerx2 = bestmat[0].trans2d(Vec2D(0, 0)).x;
				float order = (centerx2 > centerx1 ? 1 : -1);
				for (int k = 0; k < 3; ++k) {
					if (fabs(slope) < config::SLOPE_PLAIN) break;
					newfactor += (slope < 0 ? order : -order) / (5 * pow(2, k));
					slope = update_h_factor(newfactor, minslope, bestfactor, bestmat);
				}
			}
			fprintf(stderr, "Best hfactor: %lf\n", bestfactor);
			best_factor = bestfactor;
			HipCylinderWarper warper(bestfactor);
			// :65-67: the pixels into device canvases, the keypoints in place; the ImageRef sizes stay what load() left
			free_warped();
			warped.assign((size_t)n, nullptr);
			for (int k = 0; k < n; ++k) {
				op_image im{imgs[k].img ? imgs[k].img->ptr() : nullptr, imgs[k].height(), imgs[k].width(), 0, OP_F32};
				if (feats.views) PANO_HIP_CHECK(op_views_image(feats.views.get(), k, &im));
				PANO_HIP_CHECK(op_cyl_warp(ctx, &cfg, &im, (double)bestfactor, &warped[k]));
				Shape2D shape = imgs[k].shape();
				warper.warp(shape, keypoints[k]);
			}

			// accumulate
			for (int k = mid + 1; k < n; ++k) bundle.component[k].homo = bestmat[k - mid - 1];
			if (mid > 0) {      // :72-83, one call: pair (i + 1, i) with the reversed list, the ImageRefs' stale shapes
				std::vector<int> pairs, shapes;                     // over views 0 .. mid, the only ones these pairs read
				for (int i = 0; i < mid; ++i) { pairs.push_back(i + 1); pairs.push_back(i); }
				for (int i = 0; i <= mid; ++i) { shapes.push_back(imgs[i].width()); shapes.push_back(imgs[i].height()); }
				std::vector<Homography> homo;
				const int failed = estimate(left_matches.get(), keypoints.data(), mid + 1, pairs, shapes, homo);
				// Can match before, but not here. This would be a bug.
				if (failed >= 0) { fprintf(stderr, "error: Failed to match between image %d and %d.\n", failed, failed + 1); exit(1); }
				for (int i = 0; i < mid; ++i) bundle.component[i].homo = homo[i];
			}
			for (int i = mid - 2; i >= 0; --i) bundle.component[i].homo = bundle.component[i + 1].homo * bundle.component[i].homo;
			bundle.calc_inverse_homo();
			right_matches.reset(); left_matches.reset();
		}

		// cylstitcher.cc:89-137
		float update_h_factor(float nowfactor, float& minslope, float& bestfactor, std::vector<Homography>& mat) {
			const int n = (int)imgs.size(), mid = bundle.identity_idx;
			const int start = mid, end = n, len = end - start;
			std::vector<int> shapes;                                // nowimgs[k].shape() after the warp
			std::vector<std::vector<Vec2D>> nowkpts(keypoints.begin() + start, keypoints.begin() + end);
			HipCylinderWarper warper(nowfactor);
			for (int k = 0; k < len; ++k) {
				Shape2D s = imgs[start + k].shape();
				warper.warp(s, nowkpts[k]);
				shapes.push_back(s.w); shapes.push_back(s.h);
			}
			std::vector<int> pairs;                                 // in nowimgs' numbering: only views start .. n - 1 go up
			for (int k = 1; k < len; ++k) { pairs.push_back(k - 1); pairs.push_back(k); }
			std::vector<Homography> nowmat;                         // size = len - 1
			const bool failed = estimate(right_matches.get(), nowkpts.data(), len, pairs, shapes, nowmat) >= 0;
			if (failed) { attempts.push_back(Attempt{nowfactor, 0.f, false}); return 0; }
			for (int k = 1; k < len - 1; ++k) nowmat[k] = nowmat[k - 1] * nowmat[k];    // transform to nowimgs[0] == imgs[mid]
			// check the slope of the result image
			const Vec2D center2 = nowmat.back().trans2d(Vec2D(0, 0));
			const float slope = center2.y / center2.x;
			fprintf(stderr, "slope: %lf\n", slope);
			attempts.push_back(Attempt{nowfactor, slope, true});
			const float aslope = fabs(slope);
			if (aslope < minslope) {                                // update_min(minslope, fabs(slope))
				minslope = aslope;
				bestfactor = nowfactor;
				mat = std::move(nowmat);
			}
			return slope;
		}

		// bundle.blend() (stitcher_image.cc:116-155) from the pre-warped canvases, flat projection; honours config::MULTIBAND
		op_canvas* blend() {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			const int n = (int)imgs.size();
			op_blend_geom g;
			hip_bundle_geom(bundle, g);
			std::vector<op_blend_image> ims((size_t)n);
			for (int i = 0; i < n; ++i) {
				auto& c = bundle.component[i];
				ims[i].data = op_canvas_device(warped[i]); ims[i].on_device = OP_SRC_DEVICE;
				ims[i].h = c.imgptr->height(); ims[i].w = c.imgptr->width();
				PANO_HIP_CHECK(op_canvas_dims(warped[i], &ims[i].mat_h, &ims[i].mat_w));
				hip_component_geom(c, ims[i]);
			}
			op_canvas* cv = nullptr;
			PANO_HIP_CHECK(op_blend(ctx, &cfg, &g, ims.data(), n, &cv));
			return cv;
		}

		// cylstitcher.cc:139-180; records corners and inv
		op_canvas* perspective_correction(const op_canvas* img) { return hip_perspective_correction(bundle, img, corners, inv); }

	private:
		HipMatches right_matches, left_matches;                         // alive inside build_warp only
		void free_warped() { for (op_canvas* c : warped) op_canvas_free(c); warped.clear(); }
		// One op_ransac_pairs over coordinates-only features (INTEGRATION hook 3) of the n views the pairs read: kpts and (w, h)
		// per view, the pair list that goes with `m`, all three in the numbering of those n views.  homo[p] = the estimate of
		// pair p; returns the second view of the first pair that failed, -1 when none did
		int estimate(const op_matches* m, const std::vector<Vec2D>* kpts, int n, const std::vector<int>& pairs, const std::vector<int>& shapes,
				std::vector<Homography>& homo) {
			op_ctx* ctx = HipContext::get();
			const op_config cfg = hip_config_snapshot();
			const int np = (int)pairs.size() / 2;
			std::vector<const std::vector<Vec2D>*> lists;
			for (int k = 0; k < n; ++k) lists.push_back(&kpts[k]);
			const HipFeatures f = hip_features_from_keypoints(ctx, lists);
			const std::vector<uint32_t> seeds((size_t)np, base_seed);
			HipRansac r;
			PANO_HIP_CHECK(op_ransac_pairs(ctx, &cfg, f.get(), m, pairs.data(), np, shapes.data(), seeds.data(), 0, hip_out(r)));
			homo.assign((size_t)np, Homography::I());
			int failed = -1;
			for (int p = 0; p < np; ++p) {
				if (!op_ransac_ok(r.get(), p)) { if (failed < 0) failed = pairs[2 * p + 1]; continue; }
				PANO_HIP_CHECK(op_ransac_homo(r.get(), p, homo[p].data));
			}
			return failed;
		}
};

// standalone builds read like the reference
using Stitcher = HipStitcher;
using CylinderStitcher = HipCylinderStitcher;
using SIFTDetector = HipSIFTDetector;
using PairWiseMatcher = HipPairWiseMatcher;
using TransformEstimation = HipTransformEstimation;
using CylinderWarper = HipCylinderWarper;
#endif

}	// namespace pano
