// tests/harness/jpeg_write_selftest.cc -- hip_write_jpeg (openpano_amd/host/pano_hip.hh) from a plain C++ host, both overloads:
//   jpeg_write_selftest <in.bin> <out.jpg> <canvas.jpg> <canvas.bin>
// in.bin: int32 h, w ; h*w*3 float32 (Mat32f layout, Color::NO = -1 allowed).  out.jpg = hip_write_jpeg(fname, Mat32f) of that
// matrix at the defaults (quality 90, 4:2:0).  canvas.jpg = hip_write_jpeg(fname, op_canvas*, 100, OP_JPEG_444) of the
// matrix's cylinder pre-warp, a device canvas with Color::NO around the content; canvas.bin = int32 h, w and the same canvas
// as fp32.  tests/test_gpu_jpeg.py builds and checks it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pano_hip.hh"

using namespace pano;

int main(int argc, char** argv) {
	if (argc != 5) { fprintf(stderr, "usage: %s in.bin out.jpg canvas.jpg canvas.bin\n", argv[0]); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	int32_t hw[2];
	if (fread(hw, 4, 2, f) != 2) return 2;
	Mat32f mat(hw[0], hw[1], 3);
	const size_t n = (size_t)hw[0] * hw[1] * 3;
	if (fread(mat.ptr(), sizeof(float), n, f) != n) return 2;
	fclose(f);
	hip_write_jpeg(argv[2], mat);

	const op_config cfg = hip_config_snapshot();
	const op_image im = {mat.ptr(), hw[0], hw[1], 0, OP_F32};
	op_canvas* cv = nullptr;
	PANO_HIP_CHECK(op_cyl_warp(HipContext::get(), &cfg, &im, 1.0, &cv));
	hip_write_jpeg(argv[3], cv, 100, OP_JPEG_444);
	int32_t chw[2];
	PANO_HIP_CHECK(op_canvas_dims(cv, &chw[0], &chw[1]));
	std::vector<float> px((size_t)chw[0] * chw[1] * 3);
	PANO_HIP_CHECK(op_canvas_copy(HipContext::get(), cv, px.data()));
	op_canvas_free(cv);
	FILE* fo = fopen(argv[4], "wb");
	if (!fo || fwrite(chw, 4, 2, fo) != 2 || fwrite(px.data(), sizeof(float), px.size(), fo) != px.size() || fclose(fo) != 0) { perror(argv[4]); return 2; }
	return 0;
}
