// jpeg_dec_fuzz.cc -- the JPEG decoder of openpano_amd/csrc/jpeg_dec.hip run on the host: the library's header parser
// (jpeg_dec_parse.hpp) and the kernels' passes written as loops over the same jpeg_dec_core.hpp text (marker scan, passes A / B
// in Jacobi rounds, pass C, DC prediction, IDCT, upsampling, colour).  Two builds (tests/jpeg_dec_cases.py):
//   -DJPEG_DEC_MODEL_LIB  a shared library: jpeg_dec_model() gives the exit state of every subsequence after the
//                         synchronisation, the rounds it took and the pixels, for tests/test_jpeg_dec_cpu.py;
//   default               a stand-alone program for -fsanitize=address,undefined: every file named on the command line is
//                         decoded, and the first three are also put through 2000 seeded mutations (byte flips,
//                         truncations, spliced segments).  Exit 0 when every input was either decoded or refused.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "jpeg_dec_parse.hpp"

struct Model {
	uint32_t err = 0; int rounds = 0, maxl = 0, h = 0, w = 0;
	std::vector<uint32_t> states;      // 4 per subsequence: position, block in MCU, zigzag position, blocks completed
	std::vector<uint8_t> rgb;
	std::string why;
};

// JD_OK / JD_INVALID / JD_UNSUPPORTED from the parser; with JD_OK, M.err is the device's error word
static int model_decode(const unsigned char* f, int64_t size, uint32_t S, Model& M) {
	static const uint8_t zz_nat[64] = JD_ZZ_NAT;
	JdHeader H;
	const int r = jd_parse(f, size, H);
	M.why = H.why;
	if (r != JD_OK) return r;
	JdImage I;
	jd_describe(H, I);
	M.h = I.h; M.w = I.w;
	const unsigned char* src = f + H.scan_begin;
	const uint32_t n = I.in_len, nint = I.nint;
	// ---- k_jd_scan
	std::vector<uint8_t> cmp((size_t)n + JD_PAD, 0);
	std::vector<uint32_t> iv((size_t)nint + 1, 0), sf((size_t)nint + 1, 0);
	uint32_t ok = 0, om = 0, err = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t b = src[i], prev = i ? src[i - 1] : 0;
		if (b == 0xFF) {
			const uint32_t nx = i + 1 < n ? src[i + 1] : 0xFF;
			if (nx == 0) cmp[ok++] = 0xFF;
			else if ((nx & 0xF8) == 0xD0) {
				++om;
				if (nx != 0xD0 + ((om - 1) & 7)) err |= JD_ERR_MARKER;
				if (om < nint) iv[om] = ok; else err |= JD_ERR_INTERVALS;
			} else { err |= JD_ERR_MARKER; cmp[ok++] = 0xFF; }
		} else if (!(prev == 0xFF && (b == 0 || (b & 0xF8) == 0xD0))) cmp[ok++] = (uint8_t)b;
	}
	if (om + 1 != nint) err |= JD_ERR_INTERVALS;
	iv[nint] = ok;
	if (err) { M.err = err; return JD_OK; }
	uint32_t nsub = 0, maxl = 0;
	for (uint32_t j = 0; j < nint; ++j) {
		const uint32_t ns = jd_nsub(8u * (iv[j + 1] - iv[j]), S);
		sf[j] = nsub; nsub += ns; maxl = ns > maxl ? ns : maxl;
	}
	sf[nint] = nsub;
	M.maxl = (int)maxl;
	const uint32_t sub_cap = (uint32_t)(((unsigned long long)n * 8 + S - 1) / S) + nint;
	if (nsub > sub_cap) { M.err = JD_ERR_CAP; return JD_OK; }
	// ---- k_jd_sync: every subsequence of a round reads what the round before stored
	std::vector<uint32_t> of_iv(nsub);
	for (uint32_t j = 0; j < nint; ++j) for (uint32_t s = sf[j]; s < sf[j + 1]; ++s) of_iv[s] = j;
	std::vector<uint64_t> A(nsub, 0), B(nsub, 0);
	const uint8_t* d = cmp.data();
	const int bpm = (int)I.bpm;
	for (uint32_t round = 0; round < (maxl > 1 ? maxl : 1u); ++round) {
		int any = 0;
		for (uint32_t s = 0; s < nsub; ++s) {
			const uint64_t own = round ? A[s] : 0, pred = round && s ? A[s - 1] : 0;
			const uint32_t j = of_iv[s], l = s - sf[j], b0 = 8u * iv[j], e = 8u * iv[j + 1];
			const uint32_t sb = b0 + l * S, se = e - sb > S ? sb + S : e;
			B[s] = jd_sub_round(d, sb, se, e, l == 0, (int)round, pred, own, I.huff, I.kinfo, bpm);
			any |= (int)(B[s] & 1);
		}
		A.swap(B);
		if (round) ++M.rounds;
		if (!any) break;
	}
	M.states.resize((size_t)nsub * 4);
	std::vector<uint32_t> pex(nsub);
	uint32_t total = 0;
	for (uint32_t s = 0; s < nsub; ++s) {
		const JdCur c = jd_unpack(A[s]);
		uint32_t* o = &M.states[(size_t)s * 4];
		o[0] = c.pos; o[1] = (uint32_t)c.k; o[2] = (uint32_t)c.zz; o[3] = c.n;
		pex[s] = total; total += c.n;
	}
	// ---- k_jd_coef
	std::vector<int16_t> coef((size_t)I.nblocks * 64, 0);
	for (uint32_t s = 0; s < nsub; ++s) {
		const uint32_t j = of_iv[s], l = s - sf[j], b0 = 8u * iv[j], e = 8u * iv[j + 1];
		const uint32_t sb = b0 + l * S, se = e - sb > S ? sb + S : e;
		const bool last = s + 1 == sf[j + 1];
		const uint32_t m1 = (j + 1) * I.ri < I.nmcu ? (j + 1) * I.ri : I.nmcu, limit = m1 * I.bpm;
		uint32_t blk = j * I.ri * I.bpm + (pex[s] - pex[sf[j]]);
		JdCur c;
		if (l == 0) { c.pos = b0; c.k = 0; c.zz = 0; } else c = jd_unpack(A[s - 1]);
		c.n = 0;
		while (c.pos < se) {
			if (blk >= limit) { if (!jd_tail_is_padding(last, c, e)) err |= JD_ERR_COUNT; break; }
			int idx = 0, val = 0;
			const uint32_t fl = jd_step(d, e, I.huff, I.kinfo, bpm, c, idx, val);
			err |= fl & 0xFFu;
			if (fl & JD_COEF) coef[(size_t)blk * 64 + zz_nat[idx & 63]] = (int16_t)val;
			if (fl & JD_BLOCK_DONE) ++blk;
		}
		if (last && (blk != limit || c.zz)) err |= JD_ERR_COUNT;
	}
	if (err) { M.err = err; return JD_OK; }
	// ---- k_jd_dc
	const uint32_t ny = I.ncomp == 1 ? 1u : (uint32_t)(I.hs * I.vs);
	for (int c = 0; c < I.ncomp; ++c) {
		const uint32_t bc = c ? 1u : ny, koff = c ? ny + c - 1 : 0u;
		int acc = 0;
		for (uint32_t m = 0; m < I.nmcu; ++m)
			for (uint32_t sub = 0; sub < bc; ++sub) {
				if (sub == 0 && m % I.ri == 0) acc = 0;
				int16_t& v = coef[((size_t)m * I.bpm + koff + sub) * 64];
				acc = (int16_t)(acc + v);      // the device keeps 16 bits between tiles only through the stored value; valid files stay far inside
				v = (int16_t)acc;
			}
	}
	// ---- k_jd_idct
	std::vector<uint8_t> plane[3];
	for (int c = 0; c < I.ncomp; ++c) plane[c].assign((size_t)I.plane_w[c] * I.plane_h[c], 0);
	for (uint32_t b = 0; b < I.nblocks; ++b) {
		const uint32_t m = b / I.bpm, k = b - m * I.bpm;
		const int comp = jd_kinfo_comp(I.kinfo[k]);
		const int16_t* in = &coef[(size_t)b * 64];
		const uint8_t* q = I.q[comp];
		int ws[64];
		for (int c = 0; c < 8; ++c) {
			int o[8];
			jd_idct_pass<11>(in[c] * q[c], in[8 + c] * q[8 + c], in[16 + c] * q[16 + c], in[24 + c] * q[24 + c], in[32 + c] * q[32 + c], in[40 + c] * q[40 + c],
					in[48 + c] * q[48 + c], in[56 + c] * q[56 + c], o);
			for (int rr = 0; rr < 8; ++rr) ws[rr * 8 + c] = o[rr];
		}
		const int hsc = comp ? 1 : I.hs, sub = comp ? 0 : (int)k;
		const int bx = (int)(m % (uint32_t)I.mcuw) * hsc + sub % hsc, by = (int)(m / (uint32_t)I.mcuw) * (comp ? 1 : I.vs) + sub / hsc;
		for (int rr = 0; rr < 8; ++rr) {
			const int* w8 = ws + rr * 8;
			int o[8];
			jd_idct_pass<18>(w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7], o);
			for (int x = 0; x < 8; ++x) plane[comp][((size_t)by * 8 + rr) * I.plane_w[comp] + bx * 8 + x] = (uint8_t)jd_clamp255(o[x] + 128);
		}
	}
	// ---- k_jd_rgb
	M.rgb.resize((size_t)3 * I.h * I.w);
	const int cw = (I.w + I.hs - 1) / I.hs, ch = (I.h + I.vs - 1) / I.vs;
	for (int y = 0; y < I.h; ++y)
		for (int x = 0; x < I.w; ++x) {
			uint8_t* o = &M.rgb[3 * ((size_t)y * I.w + x)];
			const int Y = plane[0][(size_t)y * I.plane_w[0] + x];
			if (I.ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; continue; }
			jd_ycc_rgb(Y, jd_chroma(plane[1].data(), I.plane_w[1], cw, ch, I.hs, I.vs, y, x), jd_chroma(plane[2].data(), I.plane_w[2], cw, ch, I.hs, I.vs, y, x), o);
		}
	return JD_OK;
}

#ifdef JPEG_DEC_MODEL_LIB
// -> the number of subsequences; a negative parser code; or -100 with *err set when the data is corrupt
extern "C" long jpeg_dec_model(const unsigned char* f, long size, int S, uint32_t* states, long cap, unsigned char* rgb, int* rounds, int* maxl, unsigned* err) {
	Model M;
	const int r = model_decode(f, size, (uint32_t)S, M);
	*rounds = M.rounds; *maxl = M.maxl; *err = M.err;
	if (r != JD_OK) return r;
	if (M.err) return -100;
	const long nsub = (long)M.states.size() / 4;
	if (states) for (long i = 0; i < 4 * (nsub < cap ? nsub : cap); ++i) states[i] = M.states[(size_t)i];
	if (rgb) for (size_t i = 0; i < M.rgb.size(); ++i) rgb[i] = M.rgb[i];
	return nsub;
}
#else
static std::vector<unsigned char> slurp(const char* path) {
	std::vector<unsigned char> v;
	FILE* fp = fopen(path, "rb");
	if (!fp) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
	unsigned char buf[4096]; size_t n;
	while ((n = fread(buf, 1, sizeof buf, fp)) > 0) v.insert(v.end(), buf, buf + n);
	fclose(fp);
	return v;
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }

int main(int argc, char** argv) {
	static const uint32_t SS[4] = {32, 64, 256, 1024};
	long decoded = 0, refused = 0, corrupt = 0;
	std::vector<std::vector<unsigned char>> files;
	for (int i = 1; i < argc; ++i) files.push_back(slurp(argv[i]));
	auto feed = [&](const std::vector<unsigned char>& v, uint32_t S) {
		// an exact-size heap copy: a read past the end is the sanitizer's to see
		unsigned char* p = (unsigned char*)malloc(v.size() ? v.size() : 1);
		for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
		Model M;
		const int r = model_decode(p, (int64_t)v.size(), S, M);
		free(p);
		if (r != JD_OK) ++refused; else if (M.err) ++corrupt; else ++decoded;
		return r == JD_OK && !M.err;
	};
	for (size_t i = 0; i < files.size(); ++i) {
		const bool ok = feed(files[i], 64);
		printf("%s: %s\n", argv[i + 1], ok ? "decoded" : "refused");
	}
	const size_t nmut = files.size() < 3 ? files.size() : 3;
	for (int k = 0; nmut && k < 2000; ++k) {
		std::vector<unsigned char> v = files[(size_t)k % nmut];
		const uint32_t kind = rnd() % 4;
		if (kind == 0) { const int nf = 1 + (int)(rnd() % 4); for (int j = 0; j < nf; ++j) v[rnd() % v.size()] ^= (unsigned char)(1u << (rnd() % 8)); }
		else if (kind == 1) { const int nf = 1 + (int)(rnd() % 3); for (int j = 0; j < nf; ++j) v[rnd() % v.size()] = (unsigned char)rnd(); }
		else if (kind == 2) v.resize(rnd() % v.size());
		else {      // a run of another file spliced in
			const std::vector<unsigned char>& o = files[rnd() % files.size()];
			const size_t a = rnd() % o.size(), len = 1 + rnd() % 64, at = rnd() % v.size();
			for (size_t j = 0; j < len && a + j < o.size() && at + j < v.size(); ++j) v[at + j] = o[a + j];
		}
		feed(v, SS[rnd() % 4]);
	}
	printf("decoded %ld, refused by the parser %ld, corrupt data found by the passes %ld\n", decoded, refused, corrupt);
	return 0;
}
#endif
