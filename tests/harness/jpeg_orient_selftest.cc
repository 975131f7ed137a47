// tests/harness/jpeg_orient_selftest.cc -- hip_jpeg_exif and hip_read_jpeg_views(ctx, paths, true) (openpano_amd/host/pano_hip.hh)
// from a plain C++ host:
//   jpeg_orient_selftest <out.bin> <file.jpg> ...
// out.bin: per file int32 orientation, focal35 (hip_jpeg_exif), h, w (op_views_image of the view decoded upright) and the
// view's h*w*3 bytes (op_views_copy).  tests/test_gpu_jpeg_oriented.py builds and checks it.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "pano_hip.hh"

using namespace pano;

int main(int argc, char** argv) {
	if (argc < 3) { fprintf(stderr, "usage: %s out.bin file.jpg ...\n", argv[0]); return 2; }
	std::vector<std::string> paths(argv + 2, argv + argc);
	FILE* fo = fopen(argv[1], "wb");
	if (!fo) { perror(argv[1]); return 2; }
	op_views* v = hip_read_jpeg_views(HipContext::get(), paths, true);
	if (op_views_count(v) != (int)paths.size()) return 1;
	for (size_t k = 0; k < paths.size(); ++k) {
		int32_t rec[4] = {0, 0, 0, 0};
		hip_jpeg_exif(paths[k], &rec[0], &rec[1]);
		op_image im;
		PANO_HIP_CHECK(op_views_image(v, (int)k, &im));
		if (im.dtype != OP_U8) return 1;
		rec[2] = im.h; rec[3] = im.w;
		std::vector<unsigned char> px((size_t)im.h * im.w * 3);
		PANO_HIP_CHECK(op_views_copy(HipContext::get(), v, (int)k, px.data()));
		if (fwrite(rec, 4, 4, fo) != 4 || fwrite(px.data(), 1, px.size(), fo) != px.size()) { perror(argv[1]); return 2; }
	}
	op_views_free(v);
	if (fclose(fo) != 0) { perror(argv[1]); return 2; }
	return 0;
}
