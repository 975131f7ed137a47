// jpeg_exif_fuzz.cc -- the library's EXIF reader (openpano_amd/csrc/jpeg_exif.hpp) as a stand-alone program for
// -fsanitize=address,undefined (tests/test_jpeg_exif_cpu.py builds and runs it; nothing of it is loaded into Python).
// Every file named on the command line holds one crafted Exif APP1.  Each is read as it is, then put through seeded
// mutations of that segment: the file cut at every length inside the segment, the segment shortened at every length with the
// rest of the file moved up behind it, bit flips, byte changes and runs spliced in from elsewhere in the file.  Every
// candidate lives in a heap buffer of exactly its own size, so a read one byte past it is the sanitizer's to report.
// The reader must answer every one of them with JX_OK, an orientation in 1..8 and a focal length in 0..65535.
// Output: "<path>: orientation focal" per file, then "mutations N".  Exit 0 when all of that held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "jpeg_exif.hpp"

static long g_runs = 0;

// the candidate in a malloc block of exactly its size
static void run(const std::vector<unsigned char>& f, const char* what) {
	unsigned char* p = (unsigned char*)malloc(f.size() ? f.size() : 1);
	if (!p) { fprintf(stderr, "out of memory\n"); exit(3); }
	if (!f.empty()) memcpy(p, f.data(), f.size());
	JxExif X;
	const int r = jx_exif(p, (int64_t)f.size(), X);
	free(p);
	const bool soi = f.size() >= 4 && f[0] == 0xFF && f[1] == 0xD8;
	if (r != (soi ? JX_OK : JX_INVALID) || X.orientation < 1 || X.orientation > 8 || X.focal35 < 0 || X.focal35 > 65535) {
		fprintf(stderr, "%s: code %d, orientation %d, focal %d on a candidate of %zu bytes\n", what, r, X.orientation, X.focal35, f.size());
		exit(1);
	}
	++g_runs;
}

static uint32_t g_seed = 1;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

int main(int argc, char** argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]); return 2; }
	for (int a = 1; a < argc; ++a) {
		FILE* fp = fopen(argv[a], "rb");
		if (!fp) { perror(argv[a]); return 2; }
		std::vector<unsigned char> f; unsigned char buf[4096]; size_t n;
		while ((n = fread(buf, 1, sizeof buf, fp)) > 0) f.insert(f.end(), buf, buf + n);
		fclose(fp);
		JxExif X;
		if (jx_exif(f.data(), (int64_t)f.size(), X) != JX_OK) { fprintf(stderr, "%s: refused\n", argv[a]); return 1; }
		printf("%s: %d %d\n", argv[a], X.orientation, X.focal35);
		// the first APP1: [s0, s1)
		size_t s0 = 0;
		for (size_t i = 2; i + 4 <= f.size(); ++i) if (f[i] == 0xFF && f[i + 1] == 0xE1) { s0 = i; break; }
		if (!s0) { fprintf(stderr, "%s: no APP1\n", argv[a]); return 2; }
		const size_t s1 = s0 + 2 + ((size_t)f[s0 + 2] << 8 | f[s0 + 3]);
		if (s1 > f.size()) { fprintf(stderr, "%s: APP1 past the file\n", argv[a]); return 2; }
		run(f, "as it is");
		for (size_t cut = 0; cut <= s1; ++cut) run(std::vector<unsigned char>(f.begin(), f.begin() + cut), "cut file");
		for (size_t cut = s0; cut < s1; ++cut) {      // the segment loses its tail but keeps its length field: what follows is read as EXIF
			std::vector<unsigned char> g(f.begin(), f.begin() + cut);
			g.insert(g.end(), f.begin() + s1, f.end());
			run(g, "shortened segment");
		}
		g_seed = 12345u + (uint32_t)a;
		for (int k = 0; k < 800; ++k) {
			std::vector<unsigned char> g = f;
			const int kind = (int)(rnd() % 4), times = 1 + (int)(rnd() % 4);
			for (int t = 0; t < times; ++t) {
				const size_t at = s0 + rnd() % (s1 - s0);
				if (kind == 0) g[at] ^= (unsigned char)(1u << (rnd() % 8));
				else if (kind == 1) g[at] = (unsigned char)rnd();
				else if (kind == 2) g[at] = (rnd() & 1) ? 0xFF : 0x00;
				else {      // a run from elsewhere in the file, over the segment
					const size_t len = 1 + rnd() % 24, from = rnd() % f.size();
					for (size_t i = 0; i < len && at + i < s1 && from + i < f.size(); ++i) g[at + i] = f[from + i];
				}
			}
			run(g, "mutated segment");
		}
	}
	printf("mutations %ld\n", g_runs);
	return 0;
}
