// features.hip -- the feature table (op_features): what op_sift_batch returns and the matcher and RANSAC read.  Its
// constructors from host and device arrays, its accessors and copies out, and its copies between the devices of an op_group.
#include "features.hpp"
#include <thread>

FeaturesPtr new_features(int n, int device, const int* counts) {
	FeaturesPtr f(new op_features, op_features_free);
	f->n = n; f->counts.assign(n, 0); f->offsets.assign(n + 1, 0); f->device = device;
	for (int i = 0; counts && i < n; ++i) {
		if (counts[i] < 0) { op_set_error("negative count"); f.reset(); break; }
		f->counts[i] = counts[i]; f->offsets[i + 1] = f->offsets[i] + counts[i];
	}
	return f;
}

FeatView op_features_view(const op_features* f) {
	return FeatView{f->n, f->counts.data(), f->offsets.data(), f->has_desc ? f->desc : nullptr, f->device};
}

const double* op_features_coor_host(const op_features* f, op_ctx* ctx) {
	std::lock_guard<std::mutex> lk(f->h_mu);
	if (f->h_coor_valid) return f->h_coor.data();
	const int64_t total = f->offsets[f->n];
	f->h_coor.resize((size_t)std::max<int64_t>(total, 1) * 2);
	if (total) {
		hipError_t e = hipMemcpyAsync(f->h_coor.data(), f->coor, sizeof(double) * 2 * (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { op_set_error(std::string("op_features: coordinate copy failed: ") + hipGetErrorString(e)); return nullptr; }
	}
	f->h_coor_valid = true;
	return f->h_coor.data();
}

// device-to-device copy between two contexts' devices, ordered on dst's stream (xGMI peer copy when the
// devices differ; multi.hip enables direct peer access where the hardware allows it)
static hipError_t copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
	if (!bytes) return hipSuccess;
	if (dst_dev == src_dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
	return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st);
}

hipError_t FeatArrays::copy_rows(int64_t dst_row, const FeatArrays& src, int64_t src_row, size_t rows, hipStream_t st, int dst_dev, int src_dev) {
	hipError_t e = hipSuccess;
	if (desc && src.desc) e = copy_between(desc + dst_row * 128, dst_dev, src.desc + src_row * 128, src_dev, sizeof(float) * 128 * rows, st);
	if (e == hipSuccess && coor && src.coor) e = copy_between(coor + dst_row * 2, dst_dev, src.coor + src_row * 2, src_dev, sizeof(double) * 2 * rows, st);
	if (e == hipSuccess && real && src.real) e = copy_between(real + dst_row * 2, dst_dev, src.real + src_row * 2, src_dev, sizeof(double) * 2 * rows, st);
	return e;
}

// multi.hip, the all-gather of SURVEY 8(e).2 inside one process: part k holds the images [start[k], start[k+1]) of the
// job (contiguous blocks); EVERY device of the group gets the whole image-indexed table, each pulling the other
// devices' slices over its own xGMI links (one host thread per destination, all pairs of devices busy at once; no
// device relays another one's data).  tables[k] lands on ctxs[k]'s device.
int op_features_allgather_blocks(op_ctx* const* ctxs, int nctx, op_features* const* parts, const int* start, int n, op_features** tables) {
	std::vector<int> counts(n);
	std::vector<int64_t> offsets(n + 1, 0);
	for (int k = 0; k < nctx; ++k)
		for (int i = start[k]; i < start[k + 1]; ++i) counts[i] = parts[k]->counts[i - start[k]];
	for (int i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + counts[i];
	const int64_t total = offsets[n];
	const size_t cnt = (size_t)std::max<int64_t>(total, 1);
	std::vector<int> rcs(nctx, OP_OK);
	std::vector<std::string> errs(nctx);
	std::vector<std::thread> th;
	for (int k = 0; k < nctx; ++k) tables[k] = nullptr;
	for (int k = 0; k < nctx; ++k)
		th.emplace_back([&, k] {
			auto fail = [&](hipError_t e, const char* what) { errs[k] = std::string(what) + ": " + hipGetErrorString(e); rcs[k] = OP_ERR_HIP; };
			op_ctx* dst = ctxs[k];
			hipError_t e = hipSetDevice(dst->device);
			if (e != hipSuccess) return fail(e, "hipSetDevice");
			FeaturesPtr f = new_features(n, dst->device, counts.data());
			CallBlocks own({dst->stream});
			FeatArrays r;
			if ((e = r.alloc(own, cnt)) != hipSuccess) return fail(e, "pool_alloc");
			for (int s = 0; s < nctx; ++s) {
				const int src = (k + s) % nctx;                     // start with the own slice, then rotate: no hot source
				const op_features* p = parts[src];
				const size_t c = (size_t)(offsets[start[src + 1]] - offsets[start[src]]);
				if ((e = r.copy_rows(offsets[start[src]], FeatArrays::of(p), 0, c, dst->stream, dst->device, p->device)) != hipSuccess) return fail(e, "peer copy");
			}
			if ((e = own.finish()) != hipSuccess) return fail(e, "hipStreamSynchronize");
			r.hand_to(f.get(), own);
			tables[k] = f.release();
		});
	for (auto& t : th) t.join();
	int rc = OP_OK;
	for (int k = 0; k < nctx; ++k) if (rcs[k] != OP_OK && rc == OP_OK) { rc = rcs[k]; op_set_error("device " + std::to_string(k) + ": " + errs[k]); }
	if (rc != OP_OK) for (int k = 0; k < nctx; ++k) { op_features_free(tables[k]); tables[k] = nullptr; }
	return rc;
}

// multi.hip: the whole table of f on dst's device (one peer copy per array)
int op_features_replicate(op_ctx* dst, const op_features* src, op_features** out) {
	HIPCHK(hipSetDevice(dst->device));
	FeaturesPtr f = new_features(src->n, dst->device, src->counts.data());
	f->has_desc = src->has_desc;
	const int64_t total = src->offsets[src->n];
	CallBlocks own({dst->stream});
	FeatArrays r;
	HIPCHK(r.alloc(own, (size_t)std::max<int64_t>(total, 1), src->has_desc, false));
	HIPCHK(r.copy_rows(0, FeatArrays::of(src), 0, (size_t)total, dst->stream, dst->device, src->device));
	return r.deliver(f, own, out);
}
std::vector<op_features*>& op_features_replicas(op_features* f) { return f->replicas; }
int op_features_device(const op_features* f) { return f->device; }

extern "C" {

int op_features_num_images(const op_features* f) { return f ? f->n : 0; }
int op_features_count(const op_features* f, int i) { return (f && i >= 0 && i < f->n) ? f->counts[i] : 0; }
int64_t op_features_offset(const op_features* f, int i) { return (f && i >= 0 && i <= f->n) ? f->offsets[i] : 0; }
int64_t op_features_total(const op_features* f) { return f ? f->offsets[f->n] : 0; }
const float* op_features_desc_device(const op_features* f) { return f ? f->desc : nullptr; }
const double* op_features_coor_device(const op_features* f) { return f ? f->coor : nullptr; }

int op_features_copy(op_ctx* ctx, const op_features* f, int i, float* desc, double* coor) {
	if (!ctx || !f || i < 0 || i >= f->n) OP_FAIL(OP_ERR_INVALID, "op_features_copy: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	const int c = f->counts[i];
	if (c == 0) return OP_OK;
	if (desc) HIPCHK(hipMemcpyAsync(desc, f->desc + f->offsets[i] * 128, sizeof(float) * 128 * c, hipMemcpyDeviceToHost, ctx->stream));
	if (coor) HIPCHK(hipMemcpyAsync(coor, f->coor + f->offsets[i] * 2, sizeof(double) * 2 * c, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return OP_OK;
}

int op_features_copy_real(op_ctx* ctx, const op_features* f, int i, double* real) {
	if (!ctx || !f || i < 0 || i >= f->n || !real) OP_FAIL(OP_ERR_INVALID, "op_features_copy_real: bad argument");
	if (!f->real) OP_FAIL(OP_ERR_INVALID, "op_features_copy_real: features were not produced by op_sift_batch");
	HIPCHK(hipSetDevice(ctx->device));
	const int c = f->counts[i];
	if (c == 0) return OP_OK;
	HIPCHK(hipMemcpyAsync(real, f->real + f->offsets[i] * 2, sizeof(double) * 2 * c, hipMemcpyDeviceToHost, ctx->stream));
	HIPCHK(hipStreamSynchronize(ctx->stream));
	return OP_OK;
}

int op_features_from_host(op_ctx* ctx, const float* const* desc, const double* const* coor, const int* counts, int n, op_features** out) {
	if (!ctx || (!desc && !coor) || !counts || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_features_from_host: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	FeaturesPtr f = new_features(n, ctx->device, counts);
	if (!f) return OP_ERR_INVALID;
	const int64_t total = f->offsets[n];
	f->has_desc = desc != nullptr;       // coordinates only: enough for op_ransac_pairs, rejected by op_match_pairs
	CallBlocks own({ctx->stream});
	FeatArrays r;
	HIPCHK(r.alloc(own, (size_t)std::max<int64_t>(total, 1), f->has_desc, false));
	HIPCHK(hipMemsetAsync(r.coor, 0, sizeof(double) * 2 * (size_t)std::max<int64_t>(total, 1), ctx->stream));
	for (int i = 0; i < n; ++i) {
		if (!counts[i]) continue;
		if (f->has_desc) HIPCHK(hipMemcpyAsync(r.desc + f->offsets[i] * 128, desc[i], sizeof(float) * 128 * counts[i], hipMemcpyHostToDevice, ctx->stream));
		if (coor && coor[i]) HIPCHK(hipMemcpyAsync(r.coor + f->offsets[i] * 2, coor[i], sizeof(double) * 2 * counts[i], hipMemcpyHostToDevice, ctx->stream));
	}
	return r.deliver(f, own, out);
}

int op_features_adopt_device(op_ctx* ctx, const float* desc_dev, const double* coor_dev, const int* counts, int n, op_features** out) {
	if (!ctx || !desc_dev || !coor_dev || !counts || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_features_adopt_device: bad argument");
	FeaturesPtr f = new_features(n, ctx->device, counts);
	if (!f) return OP_ERR_INVALID;
	f->owns = false;
	f->desc = const_cast<float*>(desc_dev); f->coor = const_cast<double*>(coor_dev);
	*out = f.release();
	return OP_OK;
}

int op_features_from_device(op_ctx* ctx, const float* desc_dev, const double* coor_dev, const int* counts, int n, op_features** out) {
	if (!ctx || !desc_dev || !counts || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_features_from_device: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	FeaturesPtr f = new_features(n, ctx->device, counts);
	if (!f) return OP_ERR_INVALID;
	const int64_t total = f->offsets[n];
	const size_t cnt = (size_t)std::max<int64_t>(total, 1);
	CallBlocks own({ctx->stream});
	FeatArrays r;
	HIPCHK(r.alloc(own, cnt, true, false));
	HIPCHK(r.copy_rows(0, FeatArrays::of(desc_dev, coor_dev, nullptr), 0, (size_t)total, ctx->stream));
	if (!coor_dev || !total) HIPCHK(hipMemsetAsync(r.coor, 0, sizeof(double) * 2 * cnt, ctx->stream));
	return r.deliver(f, own, out);
}

void op_features_free(op_features* f) {
	if (!f) return;
	hipSetDevice(f->device);
	if (f->owns) { pool_free(f->desc); pool_free(f->coor); pool_free(f->real); }
	for (op_features* r : f->replicas) op_features_free(r);
	delete f;
}

}	// extern "C"
