// sift_host.hip -- host orchestration of the batched SIFT op (op_sift_batch / op_sift_batch_host; run_group also serves the
// staged dump of sift_dump.hip).  The plan comes from sift_plan.cc, the table it returns from features.hip.
//
// Mirrors SIFTDetector::do_detect_feature (feature/feature.cc:31-47) for n images at once:
// one launch per stage for the whole batch (grid z/y = image), everything resident in HBM,
// two small D2H reads of per-image counts (the caller needs K_i anyway).
#include "sift_host.hpp"
#include <map>
#include <mutex>

// contexts are few and long-lived; the table is shared by the host threads that own them (the
// reference calls detect_feature concurrently from OpenMP threads, stitcherbase.cc:14)
static std::map<op_ctx*, Workspace*> g_ws;
static std::mutex g_ws_mu;

static Workspace* ctx_workspace(op_ctx* c) {
	std::lock_guard<std::mutex> lk(g_ws_mu);
	auto it = g_ws.find(c);
	if (it != g_ws.end()) return it->second;
	Workspace* w = new Workspace;
	g_ws[c] = w;
	return w;
}
void op_ctx_release_workspace(op_ctx* c) {
	Workspace* w = nullptr;
	{
		std::lock_guard<std::mutex> lk(g_ws_mu);
		auto it = g_ws.find(c);
		if (it == g_ws.end()) return;
		w = it->second; g_ws.erase(it);
	}
	w->release(); delete w;
}

// the per-image argument check of the entry points
static int check_images(const char* who, const op_image* imgs, int n) {
	for (int i = 0; i < n; ++i)
		if (!imgs[i].data || imgs[i].h < 2 || imgs[i].w < 2 || (imgs[i].dtype != OP_F32 && imgs[i].dtype != OP_U8))
			OP_FAIL(OP_ERR_INVALID, std::string(who) + ": bad image " + std::to_string(i));
	return OP_OK;
}

// bytes of an image and its stride in the staging buffer (256-byte aligned)
struct ImgSize { size_t bytes, stride; };
static ImgSize img_size(const op_image& im) {
	const size_t bytes = (im.dtype == OP_U8 ? 1 : sizeof(float)) * (size_t)im.h * im.w * 3;
	return {bytes, (bytes + 255) & ~(size_t)255};
}

// The ONE constant stride >= their size at which n host images lie (a decoder's output pool, one block sliced into frames;
// a contiguous array of images: stride == size), or 0.  Such images travel in one strided copy: 38 separate 3 MB copies
// reach about half the link rate.  data(i) = image i's pixels.
template <typename Data> static ptrdiff_t constant_stride(int n, size_t bytes, Data data) {
	const ptrdiff_t s = n > 1 ? (const char*)data(1) - (const char*)data(0) : (ptrdiff_t)bytes;
	bool ok = s >= (ptrdiff_t)bytes;
	for (int i = 2; i < n && ok; ++i) ok = (const char*)data(i) - (const char*)data(i - 1) == s;
	return ok ? s : 0;
}

#ifndef OP_RW_SEG
#define OP_RW_SEG 0      // a build with -DOP_RW_SEG=<rows> pins the row kernel's segment height (A/B runs); 0: build_plan chooses
#endif

int run_group(op_ctx* ctx, CallBlocks& own, const op_config& cfg, const std::vector<const op_image*>& imgs, Workspace& W,
		SiftPlan& plan, FeatArrays& res, op_sift_dump* keep) {
	const int n = (int)imgs.size();
	const int sh = imgs[0]->h, sw = imgs[0]->w;
	int rc = build_plan(cfg, n, sh, sw, plan, ctx->num_cu, OP_RW_SEG);
	if (rc != OP_OK) return rc;
	if (pyramid_lds_bytes(plan.halo) > 160 * 1024 - 256) OP_FAIL(OP_ERR_UNSUPPORTED, "Gaussian halo does not fit LDS");
	hipStream_t st = ctx->stream;
	// per-image capacity of the raw / refined lists: speculative like capK below.  The kernels clamp
	// their writes and keep counting; a batch whose densest image outgrew the capacity grows the
	// buffers to the observed maximum and re-runs once (the reference has no such limit:
	// extrema.cc:36-61 appends to std::vectors).  The capacity sticks to the context.
	const int cap = W.raw_cap;
	plan.desc_list_cap = W.desc_list_cap;

	// --- buffers
	HIPCHK(W.ws.ensure(sizeof(float) * (size_t)plan.ws_stride * n));
	if (keep) HIPCHK(W.work.ensure(sizeof(float) * (size_t)plan.wh * plan.ww * 3 * n));
	HIPCHK(W.srcs.ensure(sizeof(float*) * n));
	HIPCHK(W.raw.ensure(sizeof(int) * 4 * (size_t)cap * n));
	// batch total (64 bits) | raw | refined | oriented (the block the host reads) | padding to a line | k_orientation's counters, one per line
	const size_t cnt_hdr = ((3 * (size_t)n + 2) + 31) & ~(size_t)31;
	HIPCHK(W.counts.ensure(sizeof(int) * (cnt_hdr + (size_t)n * OP_OCNT_STRIDE)));
	HIPCHK(W.refinedA.ensure(sizeof(KeyPoint) * (size_t)cap * n));
	HIPCHK(W.refinedB.ensure(sizeof(KeyPoint) * (size_t)cap * n));
	HIPCHK(W.dirs.ensure(sizeof(float) * 36 * (size_t)cap * n));
	HIPCHK(W.ndirs.ensure(sizeof(int) * (size_t)cap * n));
	HIPCHK(W.slot_of.ensure(sizeof(int) * (size_t)cap * n));
	const size_t pin_need = sizeof(long long) * (size_t)(8 * n + 16);
	if (W.pinned_cap < pin_need) {
		if (W.pinned) hipHostFree(W.pinned);
		HIPCHK(hipHostMalloc(&W.pinned, pin_need));
		W.pinned_cap = pin_need;
	}
	plan.ws = (float*)W.ws.p; plan.work = (float*)W.work.p;

	// --- sources: device pointers as they are, host images staged through one H2D copy each
	plan.src_u8 = imgs[0]->dtype == OP_U8 ? 1 : 0;
	const auto [img_bytes, img_stride] = img_size(*imgs[0]);
	size_t host_bytes = 0;
	for (auto* im : imgs) if (!im->on_device) host_bytes += img_stride;
	if (host_bytes) HIPCHK(W.staging.ensure(host_bytes));
	{
		const void** hs = (const void**)W.pinned;
		// several images, all on the host and at one constant stride: ONE copy.  Any other arrangement is copied image by image.
		const bool all_host = host_bytes == img_stride * (size_t)n && n > 1;
		const ptrdiff_t hstride = all_host ? constant_stride(n, img_bytes, [&](int i) { return imgs[i]->data; }) : 0;
		if (hstride) {
			if ((size_t)hstride == img_stride) HIPCHK(hipMemcpyAsync(W.staging.p, imgs[0]->data, img_stride * (size_t)(n - 1) + img_bytes, hipMemcpyHostToDevice, st));
			else HIPCHK(hipMemcpy2DAsync(W.staging.p, img_stride, imgs[0]->data, (size_t)hstride, img_bytes, (size_t)n, hipMemcpyHostToDevice, st));
			for (int i = 0; i < n; ++i) hs[i] = (char*)W.staging.p + (size_t)i * img_stride;
		} else {
			size_t so = 0;
			for (int i = 0; i < n; ++i) {
				if (imgs[i]->on_device) hs[i] = imgs[i]->data;
				else {
					void* d = (char*)W.staging.p + so;
					HIPCHK(hipMemcpyAsync(d, imgs[i]->data, img_bytes, hipMemcpyHostToDevice, st));
					hs[i] = d; so += img_stride;
				}
			}
		}
		// the pointer table only travels when it differs from the one the device already holds (a caller that keeps
		// its images resident passes the same pointers batch after batch)
		if (W.srcs_dev != W.srcs.p || W.srcs_last.size() != (size_t)n || !std::equal(W.srcs_last.begin(), W.srcs_last.end(), hs)) {
			HIPCHK(hipMemcpyAsync(W.srcs.p, hs, sizeof(void*) * n, hipMemcpyHostToDevice, st));
			W.srcs_last.assign(hs, hs + n); W.srcs_dev = W.srcs.p;
		}
	}
	plan.srcs = (const void* const*)W.srcs.p;

	long long* d_total = (long long*)W.counts.p;
	int* d_raw_count = (int*)W.counts.p + 2;
	int* d_refined_count = d_raw_count + n;
	int* d_oriented_count = d_raw_count + 2 * n;
	int* d_ocnt = (int*)W.counts.p + cnt_hdr;
	plan.num_cu = ctx->num_cu;
	plan.zero = (int*)W.counts.p; plan.zero_n = (int)(cnt_hdr + (size_t)n * OP_OCNT_STRIDE);      // cleared by k_grey_octaves

	{ ProfScope ps(ctx, "resize + octave grey"); HIPCHK(launch_grey_octaves(plan, keep != nullptr, st)); }
	{ ProfScope ps(ctx, "build pyramid"); HIPCHK(launch_pyramid(plan, (int*)W.raw.p, d_raw_count, cap, st)); }
	{ ProfScope ps(ctx, "extrema refine");
	  HIPCHK(launch_refine(plan, (const int*)W.raw.p, d_raw_count, cap, W.last_raw_max, (KeyPoint*)W.refinedA.p, d_refined_count, st)); }
	{ ProfScope ps(ctx, "orientation");       // histograms + peaks on the unsorted list; the canonical order (refinedB, slot_of) beside them
	  HIPCHK(launch_orientation(plan, (const KeyPoint*)W.refinedA.p, d_refined_count, cap, W.last_refined_max, (float*)W.dirs.p, (int*)W.ndirs.p, d_ocnt,
				(KeyPoint*)W.refinedB.p, (int*)W.slot_of.p, st)); }

	// The descriptor count is only known on the device at this point.  Instead of a round trip,
	// the output buffers get a capacity predicted from the previous call of this context (x1.25,
	// at least 2048 per image), output offsets and the total are computed on the device and the remaining stages are
	// enqueued right away; ONE synchronisation at the end returns the counts, and a batch that
	// outgrew the prediction re-runs its last two stages with exact sizes.
	long long capK = std::max<long long>((long long)n * 2048, W.last_total + W.last_total / 4);
	long long* h_total = (long long*)((char*)W.pinned + 16 * (size_t)n);     // pinned: [16n, ..) the counter block as it lies on the device
	int* h_counts = (int*)h_total + 2;
	long long total = 0;
	for (int attempt = 0; attempt < 2; ++attempt) {
		HIPCHK(W.oriented.ensure(sizeof(KeyPoint) * (size_t)capK));
		HIPCHK(res.alloc(own, (size_t)capK));
		{ ProfScope ps(ctx, "orientation");
		  HIPCHK(launch_expand_oriented(plan, (const KeyPoint*)W.refinedB.p, (const int*)W.slot_of.p, d_refined_count, cap, (const float*)W.dirs.p,
					(const int*)W.ndirs.p, d_ocnt, d_total, d_oriented_count, (KeyPoint*)W.oriented.p, capK, st)); }
		{ ProfScope ps(ctx, "sift descriptor");
		  HIPCHK(launch_descriptor(plan, (const KeyPoint*)W.oriented.p, d_total, capK, res.desc, res.coor, res.real, st)); }
		HIPCHK(hipMemcpyAsync(h_total, W.counts.p, sizeof(int) * (3 * (size_t)n + 2), hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		total = *h_total;
		if (total <= capK) break;
		res.drop(own);
		capK = total;                                   // exact size, second and last attempt
	}
	resolve_profile(ctx);
	W.last_total = total;
	std::vector<int> raw_count(h_counts, h_counts + n), refined_count(h_counts + n, h_counts + 2 * n);
	W.last_raw_max = *std::max_element(raw_count.begin(), raw_count.end());
	W.last_refined_max = *std::max_element(refined_count.begin(), refined_count.end());
	res.counts.assign(h_counts + 2 * n, h_counts + 3 * n);
	res.total = total;
	if (const int mx = W.last_raw_max; mx > cap) {
		if (mx > (1 << 26)) OP_FAIL(OP_ERR_CAPACITY, "raw extrema list overflow: " + std::to_string(mx));
		res.drop(own);
		W.raw_cap = mx + mx / 4 + 64;          // counts are deterministic: the re-run cannot overflow again
		return run_group(ctx, own, cfg, imgs, W, plan, res, keep);
	}
	return keep ? sift_dump_keep(keep, W, cap, res, raw_count[0], refined_count[0]) : OP_OK;
}

extern "C" {

int op_sift_batch(op_ctx* ctx, const op_config* cfg, const op_image* imgs, int n, op_features** out) {
	if (!ctx || !cfg || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_sift_batch: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	if (int rc = check_images("op_sift_batch", imgs, n)) return rc;
	// group by (size, element type), keep first-appearance order
	std::vector<std::pair<std::pair<int, int>, std::vector<int>>> groups;
	for (int i = 0; i < n; ++i) {
		std::pair<int, int> key(imgs[i].h * 2 + imgs[i].dtype, imgs[i].w);
		bool found = false;
		for (auto& g : groups) if (g.first == key) { g.second.push_back(i); found = true; break; }
		if (!found) groups.push_back({key, {i}});
	}
	Workspace* W = ctx_workspace(ctx);
	FeaturesPtr f = new_features(n, ctx->device);
	CallBlocks own({ctx->stream});
	std::vector<FeatArrays> results(groups.size());
	for (size_t g = 0; g < groups.size(); ++g) {
		std::vector<const op_image*> gi;
		for (int idx : groups[g].second) gi.push_back(&imgs[idx]);
		SiftPlan plan;
		int rc = run_group(ctx, own, *cfg, gi, *W, plan, results[g], nullptr);
		if (rc != OP_OK) return rc;
		for (size_t k = 0; k < gi.size(); ++k) f->counts[groups[g].second[k]] = results[g].counts[k];
	}
	int64_t total = 0;
	for (int i = 0; i < n; ++i) { f->offsets[i] = total; total += f->counts[i]; }
	f->offsets[n] = total;
	FeatArrays all;                              // several groups: their results in image order
	if (groups.size() == 1) own.settled();        // run_group ends behind a wait for the stream
	else {
		HIPCHK(all.alloc(own, (size_t)std::max<int64_t>(total, 1)));
		for (size_t g = 0; g < groups.size(); ++g) {
			long long go = 0;
			for (size_t k = 0; k < groups[g].second.size(); ++k) {
				const int c = results[g].counts[k];
				HIPCHK(all.copy_rows(f->offsets[groups[g].second[k]], results[g], go, (size_t)c, ctx->stream));
				go += c;
			}
		}
		HIPCHK(own.finish());
	}
	(groups.size() == 1 ? results[0] : all).hand_to(f.get(), own);
	*out = f.release();
	return OP_OK;
}

// StitcherBase::calc_feature end to end for HOST images (stitch/stitcherbase.cc:9-27: Mat32f in host memory in,
// descriptors and keypoints in host memory out) as a three-stage pipeline over chunks of the batch: the uploads of
// all chunks are queued on a copy stream at once, the kernels of chunk k start when its upload has landed, and its
// results leave on a second copy stream while chunk k+1 computes -- PCIe in, kernels and PCIe out overlap instead of
// running back to back.  Images of one size and element type (the usual job); anything else takes op_sift_batch.
int op_sift_batch_host(op_ctx* ctx, const op_config* cfg, const op_image* imgs, int n,
		float* desc_out, double* coor_out, int64_t capacity_rows, op_features** out) {
	if (!ctx || !cfg || !imgs || n <= 0 || !out || capacity_rows < 0) OP_FAIL(OP_ERR_INVALID, "op_sift_batch_host: bad argument");
	if (int rc = check_images("op_sift_batch_host", imgs, n)) return rc;
	bool uniform = true;
	for (int i = 0; i < n; ++i) uniform = uniform && !imgs[i].on_device && imgs[i].h == imgs[0].h && imgs[i].w == imgs[0].w && imgs[i].dtype == imgs[0].dtype;
	HIPCHK(hipSetDevice(ctx->device));
	const int nchunks = uniform ? std::max(1, std::min(6, n / 8)) : 1;
	if (nchunks == 1) {                      // nothing to overlap: the plain call, then one copy out
		int rc = op_sift_batch(ctx, cfg, imgs, n, out);
		if (rc != OP_OK) return rc;
		const int64_t total = (*out)->offsets[n];
		if ((desc_out || coor_out) && total > capacity_rows) OP_FAIL(OP_ERR_CAPACITY, "op_sift_batch_host: " + std::to_string(total) + " descriptors, room for " + std::to_string(capacity_rows));
		if (desc_out && total) HIPCHK(hipMemcpyAsync(desc_out, (*out)->desc, sizeof(float) * 128 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
		if (coor_out && total) HIPCHK(hipMemcpyAsync(coor_out, (*out)->coor, sizeof(double) * 2 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
		HIPCHK(hipStreamSynchronize(ctx->stream));
		return OP_OK;
	}
	HIPCHK(ctx->copy_streams());
	Workspace* W = ctx_workspace(ctx);
	const auto [img_bytes, img_stride] = img_size(imgs[0]);
	HIPCHK(W->staging.ensure(img_stride * (size_t)n));
	std::vector<int> cb(nchunks + 1, 0);
	for (int k = 0; k < nchunks; ++k) cb[k + 1] = cb[k] + n / nchunks + (k < n % nchunks ? 1 : 0);
	// constant host stride -> one (strided) copy per chunk
	const ptrdiff_t hstride = constant_stride(n, img_bytes, [&](int i) { return imgs[i].data; });
	std::vector<FeatArrays> results(nchunks);
	FeaturesPtr f = new_features(n, ctx->device);
	CallBlocks own({ctx->h2d_stream, ctx->d2h_stream, ctx->stream});       // the chunk results, the table of the batch, the events
	for (int k = 0; k < nchunks; ++k) {
		char* dst = (char*)W->staging.p + (size_t)cb[k] * img_stride;
		const int m = cb[k + 1] - cb[k];
		if (hstride) HIPCHK(hipMemcpy2DAsync(dst, img_stride, imgs[cb[k]].data, (size_t)hstride, img_bytes, (size_t)m, hipMemcpyHostToDevice, ctx->h2d_stream));
		else for (int i = 0; i < m; ++i) HIPCHK(hipMemcpyAsync(dst + (size_t)i * img_stride, imgs[cb[k] + i].data, img_bytes, hipMemcpyHostToDevice, ctx->h2d_stream));
		HIPCHK(own.event());
		HIPCHK(hipEventRecord(own.events.back(), ctx->h2d_stream));
	}
	int64_t rows = 0;
	bool overflow = false;
	for (int k = 0; k < nchunks; ++k) {
		const int m = cb[k + 1] - cb[k];
		std::vector<op_image> dev(m);
		std::vector<const op_image*> gi(m);
		for (int i = 0; i < m; ++i) {
			dev[i] = imgs[cb[k] + i]; dev[i].data = (char*)W->staging.p + (size_t)(cb[k] + i) * img_stride; dev[i].on_device = 1;
			gi[i] = &dev[i];
		}
		HIPCHK(hipStreamWaitEvent(ctx->stream, own.events[k], 0));
		SiftPlan plan;
		int rc = run_group(ctx, own, *cfg, gi, *W, plan, results[k], nullptr);
		if (rc != OP_OK) return rc;
		for (int i = 0; i < m; ++i) f->counts[cb[k] + i] = results[k].counts[i];
		const int64_t t = results[k].total;
		if ((desc_out || coor_out) && rows + t > capacity_rows) overflow = true;
		if (!overflow && t) {
			if (desc_out) HIPCHK(hipMemcpyAsync(desc_out + rows * 128, results[k].desc, sizeof(float) * 128 * (size_t)t, hipMemcpyDeviceToHost, ctx->d2h_stream));
			if (coor_out) HIPCHK(hipMemcpyAsync(coor_out + rows * 2, results[k].coor, sizeof(double) * 2 * (size_t)t, hipMemcpyDeviceToHost, ctx->d2h_stream));
		}
		rows += t;
	}
	for (int i = 0; i < n; ++i) f->offsets[i + 1] = f->offsets[i] + f->counts[i];
	{	// the resident table of the whole batch (the matcher's input): chunk results back to back
		FeatArrays all;
		HIPCHK(all.alloc(own, (size_t)std::max<int64_t>(rows, 1)));
		int64_t o = 0;
		for (int k = 0; k < nchunks; ++k) {
			HIPCHK(all.copy_rows(o, results[k], 0, (size_t)results[k].total, ctx->stream));
			o += results[k].total;
		}
		HIPCHK(own.finish());
		all.hand_to(f.get(), own);
	}
	*out = f.release();
	if (overflow) OP_FAIL(OP_ERR_CAPACITY, "op_sift_batch_host: " + std::to_string(rows) + " descriptors, room for " + std::to_string(capacity_rows) + " (the resident features are returned)");
	return OP_OK;
}

int op_debug_set_raw_capacity(op_ctx* ctx, int cap) {
	if (!ctx || cap < 64) OP_FAIL(OP_ERR_INVALID, "op_debug_set_raw_capacity: bad argument");
	ctx_workspace(ctx)->raw_cap = cap;
	return OP_OK;
}

int op_debug_set_desc_list_cap(op_ctx* ctx, int floats) {
	if (!ctx || floats < 0 || floats > OP_DESC_LIST_CAP) OP_FAIL(OP_ERR_INVALID, "op_debug_set_desc_list_cap: bad argument");
	ctx_workspace(ctx)->desc_list_cap = floats;
	return OP_OK;
}

}	// extern "C"
