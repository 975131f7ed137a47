// views.hip -- op_views_upload and the accessors of the resident views (struct op_views: internal.hpp)
#include "internal.hpp"

extern "C" {

// ---- op_views: the views of a job, uploaded once in the type the decoder produced, resident for SIFT, the cylinder
// warp, the overlap passes and every blend (the reference's seam: ImageRef::load / img, stitch/imageref.hh:15-31) ----
int op_views_upload(op_ctx* ctx, const op_image* imgs, int n, op_views** out) {
	if (!ctx || !imgs || n <= 0 || !out) OP_FAIL(OP_ERR_INVALID, "op_views_upload: bad argument");
	*out = nullptr;
	for (int i = 0; i < n; ++i)
		if (!imgs[i].data || imgs[i].h < 2 || imgs[i].w < 2 || (imgs[i].dtype != OP_F32 && imgs[i].dtype != OP_U8) ||
				(imgs[i].on_device != 0 && imgs[i].on_device != 1))
			OP_FAIL(OP_ERR_INVALID, "op_views_upload: bad image " + std::to_string(i));
	HIPCHK(hipSetDevice(ctx->device));
	hipStream_t st = ctx->stream;
	// every view at an offset that is a multiple of 256 bytes of ONE block
	std::vector<size_t> bytes(n), off(n);
	size_t total = 0;
	for (int i = 0; i < n; ++i) {
		bytes[i] = (imgs[i].dtype == OP_U8 ? 1 : sizeof(float)) * 3 * (size_t)imgs[i].h * imgs[i].w;
		off[i] = total; total += (bytes[i] + 255) & ~(size_t)255;
	}
	CallBlocks own({st});
	char* block = nullptr;
	HIPCHK(own.alloc(&block, total));
	// host images of one size at one constant stride (a contiguous array of frames, a decoder pool) go up in ONE copy
	bool packed = n > 1;
	for (int i = 0; i < n && packed; ++i) packed = !imgs[i].on_device && bytes[i] == bytes[0];
	ptrdiff_t hstride = packed ? (const char*)imgs[1].data - (const char*)imgs[0].data : 0;
	packed = packed && hstride >= (ptrdiff_t)bytes[0];
	for (int i = 2; i < n && packed; ++i) packed = (const char*)imgs[i].data - (const char*)imgs[i - 1].data == hstride;
	hipError_t e = hipSuccess;
	if (packed) e = hipMemcpy2DAsync(block, off[1], imgs[0].data, (size_t)hstride, bytes[0], (size_t)n, hipMemcpyHostToDevice, st);
	else for (int i = 0; i < n && e == hipSuccess; ++i)
		e = hipMemcpyAsync(block + off[i], imgs[i].data, bytes[i], imgs[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
	if (e == hipSuccess) e = own.finish();       // the caller's host buffers are free again when this returns
	if (e != hipSuccess) OP_FAIL(OP_ERR_HIP, std::string("op_views_upload: ") + hipGetErrorString(e));
	op_views* v = new op_views;
	v->ctx = ctx; v->block = own.release(block);
	v->imgs.resize(n);
	for (int i = 0; i < n; ++i) v->imgs[i] = op_image{block + off[i], imgs[i].h, imgs[i].w, 1, imgs[i].dtype};
	*out = v;
	return OP_OK;
}

int op_views_count(const op_views* v) {
	if (!v) OP_FAIL(OP_ERR_INVALID, "op_views_count: NULL views");
	return (int)v->imgs.size();
}

int op_views_image(const op_views* v, int i, op_image* out) {
	if (!v || !out || i < 0 || i >= (int)v->imgs.size()) OP_FAIL(OP_ERR_INVALID, "op_views_image: bad argument");
	*out = v->imgs[i];
	return OP_OK;
}

int op_views_blend_image(const op_views* v, int i, op_blend_image* out) {
	if (!v || !out || i < 0 || i >= (int)v->imgs.size()) OP_FAIL(OP_ERR_INVALID, "op_views_blend_image: bad argument");
	const op_image& im = v->imgs[i];
	out->data = (const float*)im.data; out->h = im.h; out->w = im.w;
	out->on_device = OP_SRC_DEVICE | (im.dtype == OP_U8 ? OP_SRC_U8 : 0);
	out->mat_h = 0; out->mat_w = 0;
	return OP_OK;
}

void op_views_free(op_views* v) {
	if (!v) return;
	// the pool does not track streams: work of the context's stream that still reads the views must be over before the
	// block can be handed to another caller
	if (v->block) {
		if (hipSetDevice(v->ctx->device) == hipSuccess) (void)hipStreamSynchronize(v->ctx->stream);
		pool_free(v->block);
	}
	delete v;
}

}	// extern "C"
