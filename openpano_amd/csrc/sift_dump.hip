// sift_dump.hip -- the staged dump (op_sift_staged): one image through run_group with every intermediate kept for the tests
// that compare the pipeline stage by stage -- planes read from the private workspace, lists copied to the host.
#include "sift_host.hpp"
#include <array>
#include <cmath>
#include <cstring>

struct op_sift_dump {
	Workspace w;                       // private workspace kept alive for plane reads
	SiftPlan plan;
	int cap = 0;
	std::vector<int> raw;              // sorted (o, s, y, x) quads: x, y, o, s
	std::vector<KeyPoint> refined, oriented;
	std::vector<float> desc; std::vector<double> coor01;
};

int sift_dump_keep(op_sift_dump* keep, const Workspace& W, int cap, const FeatArrays& res, int raw_count, int refined_count) {
	const long long total = res.total;
	keep->cap = cap;
	keep->raw.resize((size_t)raw_count * 4);
	if (raw_count) HIPCHK(hipMemcpy(keep->raw.data(), W.raw.p, sizeof(int) * 4 * raw_count, hipMemcpyDeviceToHost));
	keep->refined.resize(refined_count);
	if (refined_count) HIPCHK(hipMemcpy(keep->refined.data(), W.refinedB.p, sizeof(KeyPoint) * refined_count, hipMemcpyDeviceToHost));
	keep->oriented.resize(total);
	if (total) HIPCHK(hipMemcpy(keep->oriented.data(), W.oriented.p, sizeof(KeyPoint) * total, hipMemcpyDeviceToHost));
	keep->desc.resize((size_t)total * 128);
	if (total) HIPCHK(hipMemcpy(keep->desc.data(), res.desc, sizeof(float) * 128 * total, hipMemcpyDeviceToHost));
	// sort the raw list into scan order (o, s, y, x)
	std::vector<std::array<int, 4>> q(raw_count);
	for (int i = 0; i < raw_count; ++i) q[i] = {keep->raw[4 * i + 2], keep->raw[4 * i + 3], keep->raw[4 * i + 1], keep->raw[4 * i]};
	std::sort(q.begin(), q.end());
	for (int i = 0; i < raw_count; ++i) { keep->raw[4 * i] = q[i][3]; keep->raw[4 * i + 1] = q[i][2]; keep->raw[4 * i + 2] = q[i][0]; keep->raw[4 * i + 3] = q[i][1]; }
	return OP_OK;
}

extern "C" {

int op_sift_staged(op_ctx* ctx, const op_config* cfg, const op_image* img, op_sift_dump** out) {
	if (!ctx || !cfg || !img || !img->data || !out || (img->dtype != OP_F32 && img->dtype != OP_U8)) OP_FAIL(OP_ERR_INVALID, "op_sift_staged: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	std::unique_ptr<op_sift_dump, void (*)(op_sift_dump*)> d(new op_sift_dump, op_sift_dump_free);
	CallBlocks own({ctx->stream});
	FeatArrays res;
	std::vector<const op_image*> gi{img};
	int rc = run_group(ctx, own, *cfg, gi, d->w, d->plan, res, d.get());
	if (rc != OP_OK) return rc;
	own.settled();                              // run_group ends behind a wait for the stream
	if (res.total) {
		d->coor01.resize((size_t)res.total * 2);
		for (long long i = 0; i < res.total; ++i) { d->coor01[2 * i] = d->oriented[i].rx; d->coor01[2 * i + 1] = d->oriented[i].ry; }
	}
	*out = d.release();
	return OP_OK;
}

void op_sift_dump_free(op_sift_dump* d) { if (!d) return; d->w.release(); delete d; }

int op_sift_dump_working_dims(const op_sift_dump* d, int* h, int* w) { *h = d->plan.wh; *w = d->plan.ww; return OP_OK; }
int op_sift_dump_octave_dims(const op_sift_dump* d, int oct, int* h, int* w) {
	if (oct < 0 || oct >= d->plan.noct) OP_FAIL(OP_ERR_INVALID, "bad octave");
	*h = d->plan.oct[oct].h; *w = d->plan.oct[oct].w; return OP_OK;
}

int op_sift_dump_plane(op_ctx* ctx, const op_sift_dump* d, int kind, int oct, int s, float* out) {
	if (!ctx || !d || !out) OP_FAIL(OP_ERR_INVALID, "op_sift_dump_plane: bad argument");
	HIPCHK(hipSetDevice(ctx->device));
	const SiftPlan& p = d->plan;
	if (kind == 4) {
		HIPCHK(hipMemcpy(out, p.work, sizeof(float) * (size_t)p.wh * p.ww * 3, hipMemcpyDeviceToHost));
		return OP_OK;
	}
	if (oct < 0 || oct >= p.noct) OP_FAIL(OP_ERR_INVALID, "bad octave");
	const OctDesc& o = p.oct[oct];
	long long off;
	if (kind == 5) off = plane_off_grey(o);
	else if (kind == 1 && s >= 0 && s <= p.nscale - 2) {
		// DoG planes are never materialised by the product path (sift_plan.hpp); the dump evaluates
		// dog[s] = |G[s] - G[s+1]| (feature/dog.cc:126) on the two Gaussian planes, one fp32 subtraction per pixel
		std::vector<float> nxt((size_t)o.plane);
		HIPCHK(hipMemcpy(out, p.ws + plane_off_gauss(o, p.nscale, s), sizeof(float) * (size_t)o.plane, hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(nxt.data(), p.ws + plane_off_gauss(o, p.nscale, s + 1), sizeof(float) * (size_t)o.plane, hipMemcpyDeviceToHost));
		for (long long i = 0; i < o.plane; ++i) out[i] = std::fabs(out[i] - nxt[i]);
		return OP_OK;
	}
	else if ((kind == 2 || kind == 3) && s >= 1 && s <= p.nscale - 3) {
		// mag / ort planes are never materialised by the product path; the dump computes them
		float* tmp = nullptr;
		HIPCHK(hipMalloc(&tmp, sizeof(float) * 2 * (size_t)o.plane));
		hipError_t e = launch_magort_plane(p, 0, oct, s, tmp, tmp + o.plane, ctx->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(out, tmp + (kind == 3 ? o.plane : 0), sizeof(float) * (size_t)o.plane, hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		hipFree(tmp);
		if (e != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string("op_sift_dump_plane: ") + hipGetErrorString(e));
		return OP_OK;
	}
	else if (kind == 6 && s >= 1 && s <= p.nscale - 1) off = plane_off_gauss(o, p.nscale, s);
	else OP_FAIL(OP_ERR_INVALID, "bad plane kind/scale");
	HIPCHK(hipMemcpy(out, p.ws + off, sizeof(float) * (size_t)o.plane, hipMemcpyDeviceToHost));
	return OP_OK;
}

int op_sift_dump_raw_count(const op_sift_dump* d, int oct, int s) {
	int c = 0;
	for (size_t i = 0; i < d->raw.size() / 4; ++i) c += (d->raw[4 * i + 2] == oct && d->raw[4 * i + 3] == s);
	return c;
}
int op_sift_dump_raw(const op_sift_dump* d, int oct, int s, int* xy) {
	int c = 0;
	for (size_t i = 0; i < d->raw.size() / 4; ++i)
		if (d->raw[4 * i + 2] == oct && d->raw[4 * i + 3] == s) { xy[2 * c] = d->raw[4 * i]; xy[2 * c + 1] = d->raw[4 * i + 1]; ++c; }
	return c;
}
int op_sift_dump_kp_count(const op_sift_dump* d, int which) { return (int)(which ? d->oriented.size() : d->refined.size()); }
int op_sift_dump_kp(const op_sift_dump* d, int which, int* ints, double* real, float* fl) {
	const std::vector<KeyPoint>& v = which ? d->oriented : d->refined;
	for (size_t i = 0; i < v.size(); ++i) {
		ints[4 * i] = v[i].x; ints[4 * i + 1] = v[i].y; ints[4 * i + 2] = v[i].oct; ints[4 * i + 3] = v[i].scale;
		real[2 * i] = v[i].rx; real[2 * i + 1] = v[i].ry;
		fl[2 * i] = which ? v[i].dir : 0.f; fl[2 * i + 1] = v[i].sf;
	}
	return OP_OK;
}
int op_sift_dump_desc(const op_sift_dump* d, float* desc, double* coor) {
	if (desc && !d->desc.empty()) memcpy(desc, d->desc.data(), sizeof(float) * d->desc.size());
	if (coor && !d->coor01.empty()) memcpy(coor, d->coor01.data(), sizeof(double) * d->coor01.size());
	return OP_OK;
}

}	// extern "C"
