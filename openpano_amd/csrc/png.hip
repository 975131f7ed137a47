// png.hip -- the canvas as a PNG file, encoded on the device (C-ABI 12).
//
// Stands in for write_rgb -> write_png -> lodepng::encode (lib/imgio.cc:25-41,98-113), the largest single cost of a whole
// run of the reference's CLI.  8-bit RGB, colour type 2, no interlace: signature, IHDR, IDAT chunks, IEND.  Three kernels:
//   k_png_filter   one workgroup per scanline: quantise (sample_byte) and pick the PNG filter type with
//                  the smallest sum of |residual as a signed byte|, ties to the lowest type; writes the filtered stream F;
//   k_png_deflate  one workgroup per PNG_SEG bytes of F: hash candidates, a greedy parse of 256 sub-blocks (one per thread),
//                  dynamic Huffman tables, bits packed (LsbWriter) at offsets from a prefix sum (wg_scan_inclusive); or a stored block when that is not larger.
//                  Every segment is a byte-aligned piece of ONE deflate stream (closed by an empty stored block; the last one
//                  carries BFINAL) and becomes its own IDAT chunk, so no CRC has to be combined across segments;
//   k_png_pack     exclusive scan of the sizes (wg_slot_offset), every piece copied to its place with its chunk length / type / CRC-32; the
//                  zlib header and the Adler-32 (combined from the segments' partial sums) are IDAT chunks of their own.
// Every choice is fixed by position and value, never by lane or arrival order (LDS atomics used: add, max, or, xor on
// integers -- all commutative), so the file is a function of the pixels alone; tests/harness/png_ref.c is the same
// algorithm written serially and the GPU tests require equal bytes.  The named helpers and the file handle: codec_shared.hpp.
#include "codec_shared.hpp"

#define PNG_SEG 61440        // bytes of filtered stream per segment = 256 sub-blocks; a multiple of 3 (2 SEG + 1 is a possible length)
#define PNG_SUB 240          // bytes one thread parses; a match never crosses a sub-block's end
#define PNG_WINDOW 32768
#define PNG_HASH_BITS 13
#define PNG_TOO_FAR 4096     // a match of length 3 farther away than this costs more than three literals
#define PNG_SLOT (PNG_SEG + 16)   // worst case of a segment's deflate bytes (stored: SEG + 5), 16-byte aligned
#define PNG_ADLER 65521u
#define PNG_HEAD_BYTES 47    // signature 8, IHDR chunk 25, zlib-header chunk 14
// Code-length limits of the three Huffman alphabets.  The defaults are deflate's own; RFC 1951 bounds code lengths from above
// only, so a tighter limit still gives a valid file -- the tests build a variant with 11 / 11 / 5 to run huff_build's Kraft
// fix-up on ordinary inputs (tests/test_gpu_png_variant.py; tests/harness/png_ref.c has the same knobs).
#ifndef OP_PNG_LIT_MAXBITS
#define OP_PNG_LIT_MAXBITS 15
#endif
#ifndef OP_PNG_DIST_MAXBITS
#define OP_PNG_DIST_MAXBITS 15
#endif
#ifndef OP_PNG_CL_MAXBITS
#define OP_PNG_CL_MAXBITS 7
#endif
static_assert(OP_PNG_LIT_MAXBITS >= 9 && OP_PNG_LIT_MAXBITS <= 15, "286 codes need 9 bits; deflate allows 15");
static_assert(OP_PNG_DIST_MAXBITS >= 5 && OP_PNG_DIST_MAXBITS <= 15, "30 codes need 5 bits; deflate allows 15");
static_assert(OP_PNG_CL_MAXBITS >= 5 && OP_PNG_CL_MAXBITS <= 7, "19 codes need 5 bits; a code-length code length is a 3-bit field");

struct op_png : EncodedFile {};

namespace {

// ------------------------------------------------ filter ------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
	const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
	return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int sabs(int v) { v &= 255; return v < 128 ? v : 256 - v; }

template <typename T>
__global__ void __launch_bounds__(256) k_png_filter(const T* __restrict__ src, int h, int w, unsigned char* __restrict__ F) {
	__shared__ unsigned int sum[5];
	const int y = blockIdx.x, t = threadIdx.x;
	const long long R = 3LL * w;
	const T* cur = src + (long long)y * R;
	const T* up = y ? cur - R : nullptr;
	if (t < 5) sum[t] = 0;
	__syncthreads();
	unsigned int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
	for (long long x = t; x < R; x += 256) {
		const int v = sample_byte(cur, x), a = x >= 3 ? sample_byte(cur, x - 3) : 0, b = up ? sample_byte(up, x) : 0, c = (up && x >= 3) ? sample_byte(up, x - 3) : 0;
		s0 += sabs(v); s1 += sabs(v - a); s2 += sabs(v - b); s3 += sabs(v - ((a + b) >> 1)); s4 += sabs(v - paeth(a, b, c));
	}
	atomicAdd(&sum[0], s0); atomicAdd(&sum[1], s1); atomicAdd(&sum[2], s2); atomicAdd(&sum[3], s3); atomicAdd(&sum[4], s4);
	__syncthreads();
	int best = 0; unsigned int bs = sum[0];
	for (int k = 1; k < 5; ++k) { const unsigned int s = sum[k]; if (s < bs) { bs = s; best = k; } }
	unsigned char* o = F + (long long)y * (R + 1);
	if (t == 0) o[0] = (unsigned char)best;
	for (long long x = t; x < R; x += 256) {
		const int v = sample_byte(cur, x), a = x >= 3 ? sample_byte(cur, x - 3) : 0, b = up ? sample_byte(up, x) : 0, c = (up && x >= 3) ? sample_byte(up, x - 3) : 0;
		const int pred = best == 0 ? 0 : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : paeth(a, b, c);
		o[1 + x] = (unsigned char)(v - pred);
	}
}

// ------------------------------------------------ deflate ------------------------------------------------
struct HuffWork { uint32_t key[288]; uint16_t sym[288]; int num[33]; uint32_t next_code[17]; int used; };
struct DeflateLds {
	union { int head[1 << PNG_HASH_BITS]; uint32_t outw[PNG_SLOT / 4]; } u;   // the hash heads are dead before the output is staged
	uint32_t freq[320];          // 0..285 literal / length, 288..317 distance
	uint32_t clfreq[19];
	HuffWork hw;
	uint16_t codes[320], clcodes[19];
	uint8_t lens[320], cllens[19];
	uint8_t cls[320], clx[320];  // the code-length sequence: symbol 0..18 and the repeat count's extra bits
	int ncl, hlit, hdist, hclen;
	int nsym[256];
	uint32_t bitoff[256];
	unsigned long long adA, adB;
	uint32_t hdr_bits, size;
	int use_stored;
};

static_assert(sizeof(DeflateLds) <= 80 * 1024, "two k_png_deflate workgroups must fit a CU's 160 KiB of LDS");

__constant__ unsigned char c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ uint32_t hash3(const unsigned char* p) {
	return (((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16) * 2654435761u) >> (32 - PNG_HASH_BITS);
}
__device__ __forceinline__ void len_code(int len, int& code, int& ebits, int& eval) {
	const int l = len - 3;
	if (len == 258) { code = 285; ebits = 0; eval = 0; }
	else if (l < 8) { code = 257 + l; ebits = 0; eval = 0; }
	else { const int e = 29 - __clz(l); code = 257 + 4 * (e + 1) + ((l >> e) & 3); ebits = e; eval = l & ((1 << e) - 1); }
}
__device__ __forceinline__ void dist_code(int dist, int& code, int& ebits, int& eval) {
	const int d = dist - 1;
	if (d < 4) { code = d; ebits = 0; eval = 0; }
	else { const int e = 30 - __clz(d); code = 2 * (e + 1) + ((d >> e) & 1); ebits = e; eval = d & ((1 << e) - 1); }
}

// Code lengths (limit maxbits) and canonical codes, bit-reversed for the LSB-first stream, of n symbol counts.  Called by the
// whole workgroup; every table is in LDS.  Rank by (count, symbol), Moffat-Katajainen in-place lengths, Kraft fix-up,
// shortest lengths to the highest ranks.
__device__ void huff_build(const uint32_t* freq, int n, int maxbits, uint8_t* lens, uint16_t* codes, HuffWork& w) {
	const int t = threadIdx.x;
	if (t == 0) w.used = 0;
	for (int s = t; s < n; s += 256) { lens[s] = 0; codes[s] = 0; }
	__syncthreads();
	for (int s = t; s < n; s += 256) {
		const uint32_t f = freq[s];
		if (!f) continue;
		int r = 0;
		for (int q = 0; q < n; ++q) { const uint32_t fq = freq[q]; r += (fq && (fq < f || (fq == f && q < s))) ? 1 : 0; }
		w.key[r] = f; w.sym[r] = (uint16_t)s;
		atomicAdd(&w.used, 1);
	}
	__syncthreads();
	if (t == 0 && w.used > 0) {
		const int used = w.used;
		uint32_t* key = w.key;
		if (used == 1) key[0] = 1;
		else {
			int root = 0, leaf = 2, next, avbl = 1, usd = 0, dpth = 0;
			key[0] += key[1];
			for (next = 1; next < used - 1; ++next) {
				if (leaf >= used || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = (uint32_t)next; } else key[next] = key[leaf++];
				if (leaf >= used || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = (uint32_t)next; } else key[next] += key[leaf++];
			}
			key[used - 2] = 0;
			for (next = used - 3; next >= 0; --next) key[next] = key[key[next]] + 1;
			root = used - 2; next = used - 1;
			while (avbl > 0) {
				while (root >= 0 && (int)key[root] == dpth) { ++usd; --root; }
				while (avbl > usd) { key[next--] = (uint32_t)dpth; --avbl; }
				avbl = 2 * usd; ++dpth; usd = 0;
			}
		}
		for (int i = 0; i < 33; ++i) w.num[i] = 0;
		for (int i = 0; i < used; ++i) w.num[key[i] > 32 ? 32 : key[i]]++;
		if (used > 1) {
			uint32_t total = 0;
			for (int i = maxbits + 1; i <= 32; ++i) { w.num[maxbits] += w.num[i]; w.num[i] = 0; }
			for (int i = maxbits; i > 0; --i) total += (uint32_t)w.num[i] << (maxbits - i);
			while (total != (1u << maxbits)) {
				w.num[maxbits]--;
				for (int i = maxbits - 1; i > 0; --i) if (w.num[i]) { w.num[i]--; w.num[i + 1] += 2; break; }
				--total;
			}
		}
		for (int i = 1, j = used; i <= maxbits; ++i) for (int l = w.num[i]; l > 0; --l) lens[w.sym[--j]] = (uint8_t)i;
		uint32_t code = 0;
		w.next_code[0] = 0;
		for (int b = 1; b <= maxbits; ++b) { code = (code + (b > 1 ? (uint32_t)w.num[b - 1] : 0u)) << 1; w.next_code[b] = code; }
	}
	__syncthreads();
	if (t == 0 && w.used > 0) {
		for (int s = 0; s < n; ++s) {
			const int l = lens[s];
			if (!l) continue;
			const uint32_t c = w.next_code[l]++;
			codes[s] = (uint16_t)(__brev(c) >> (32 - l));
		}
	}
	__syncthreads();
}

__global__ void __launch_bounds__(256) k_png_deflate(const unsigned char* __restrict__ F, long long N, int nseg,
		uint16_t* __restrict__ cand_all, uint32_t* __restrict__ syms_all, unsigned char* __restrict__ slots,
		uint32_t* __restrict__ sizes, uint32_t* __restrict__ adler_a, uint32_t* __restrict__ adler_b) {
	extern __shared__ __attribute__((aligned(16))) unsigned char png_lds_raw[];
	DeflateLds& S = *reinterpret_cast<DeflateLds*>(png_lds_raw);
	const int t = threadIdx.x, seg = blockIdx.x;
	const long long s0 = (long long)seg * PNG_SEG, s1 = s0 + PNG_SEG < N ? s0 + PNG_SEG : N;
	const int L = (int)(s1 - s0);
	const bool last = seg == nseg - 1;
	uint16_t* cand = cand_all + s0;
	uint32_t* syms = syms_all + s0;
	unsigned char* slot = slots + (long long)seg * PNG_SLOT;

	for (int k = t; k < (1 << PNG_HASH_BITS); k += 256) S.u.head[k] = 0;
	for (int k = t; k < 320; k += 256) S.freq[k] = 0;
	if (t < 19) S.clfreq[t] = 0;
	if (t == 0) { S.adA = 0; S.adB = 0; }
	__syncthreads();
	// ---- hash candidates.  Positions are kept as (p - s0 + WINDOW + 1), 0 = empty; max() makes "the latest" independent of
	// the order in which the lanes arrive.  A position sees the window before the segment and the EARLIER groups of 256.
	for (long long p = (s0 - PNG_WINDOW < 0 ? 0 : s0 - PNG_WINDOW) + t; p < s0; p += 256)
		if (p + 2 < N) atomicMax(&S.u.head[hash3(F + p)], (int)(p - s0) + PNG_WINDOW + 1);
	__syncthreads();
	for (int g = 0; g < L; g += 256) {
		const int q = g + t;
		const bool hashed = q < L && s0 + q + 2 < N;
		uint32_t hh = 0;
		if (q < L) {
			uint16_t c = 0;
			if (hashed) {
				hh = hash3(F + s0 + q);
				const int hd = S.u.head[hh];
				if (hd) { const int d = (q + PNG_WINDOW + 1) - hd; if (d <= PNG_WINDOW) c = (uint16_t)d; }
			}
			cand[q] = c;
		}
		__syncthreads();
		if (hashed) atomicMax(&S.u.head[hh], q + PNG_WINDOW + 1);
		__syncthreads();
	}
	// ---- greedy parse of this thread's sub-block; Adler-32 partial sums of its bytes
	{
		long long i = s0 + (long long)t * PNG_SUB;
		const long long e = i + PNG_SUB < s1 ? i + PNG_SUB : s1;
		unsigned long long a = 0, b = 0;
		for (long long j = i; j < e; ++j) { const unsigned int v = F[j]; a += v; b += (unsigned long long)(s1 - j) * v; }
		if (i < e) { atomicAdd(&S.adA, a); atomicAdd(&S.adB, b); }
		int n = 0;
		while (i < e) {
			const int maxlen = e - i < 258 ? (int)(e - i) : 258;
			int bl = 0, bd = 0;
			for (int k = 0; k < 3; ++k) {
				const int d = k == 0 ? 1 : k == 1 ? 3 : (int)cand[i - s0];
				if (d == 0 || d > i) continue;
				int l = 0;
				while (l < maxlen && F[i + l] == F[i - d + l]) ++l;
				if (l > bl || (l == bl && l > 0 && d < bd)) { bl = l; bd = d; }
			}
			if (bl >= 3 && !(bl == 3 && bd > PNG_TOO_FAR)) {
				int c, eb, ev;
				syms[t * PNG_SUB + n++] = 0x80000000u | (uint32_t)bl << 15 | (uint32_t)(bd - 1);
				len_code(bl, c, eb, ev); atomicAdd(&S.freq[c], 1u);
				dist_code(bd, c, eb, ev); atomicAdd(&S.freq[288 + c], 1u);
				i += bl;
			} else { const unsigned int v = F[i]; syms[t * PNG_SUB + n++] = v; atomicAdd(&S.freq[v], 1u); ++i; }
		}
		S.nsym[t] = n;
	}
	__syncthreads();
	if (t == 0) {
		S.freq[256] = 1;
		bool any = false;
		for (int c = 0; c < 30; ++c) any |= S.freq[288 + c] != 0;
		if (!any) S.freq[288] = 1;      // a distance alphabet must describe at least one code
	}
	__syncthreads();
	huff_build(S.freq, 286, OP_PNG_LIT_MAXBITS, S.lens, S.codes, S.hw);
	huff_build(S.freq + 288, 30, OP_PNG_DIST_MAXBITS, S.lens + 288, S.codes + 288, S.hw);
	if (t == 0) {
		int hlit = 286, hdist = 30;
		while (hlit > 257 && !S.lens[hlit - 1]) --hlit;
		while (hdist > 1 && !S.lens[288 + hdist - 1]) --hdist;
		S.hlit = hlit; S.hdist = hdist;
		// both alphabets' lengths as one sequence, run-length coded with 16 / 17 / 18
		const int nseq = hlit + hdist;
		int ncl = 0;
		for (int k = 0; k < nseq;) {
			const int v = k < hlit ? S.lens[k] : S.lens[288 + k - hlit];
			int r = 1;
			while (k + r < nseq && (k + r < hlit ? S.lens[k + r] : S.lens[288 + k + r - hlit]) == v) ++r;
			k += r;
			if (v == 0) {
				while (r >= 11) { const int m = r < 138 ? r : 138; S.cls[ncl] = 18; S.clx[ncl++] = (uint8_t)(m - 11); r -= m; }
				if (r >= 3) { S.cls[ncl] = 17; S.clx[ncl++] = (uint8_t)(r - 3); r = 0; }
				while (r-- > 0) { S.cls[ncl] = 0; S.clx[ncl++] = 0; }
			} else {
				S.cls[ncl] = (uint8_t)v; S.clx[ncl++] = 0; --r;
				while (r >= 3) { const int m = r < 6 ? r : 6; S.cls[ncl] = 16; S.clx[ncl++] = (uint8_t)(m - 3); r -= m; }
				while (r-- > 0) { S.cls[ncl] = (uint8_t)v; S.clx[ncl++] = 0; }
			}
		}
		S.ncl = ncl;
		for (int k = 0; k < ncl; ++k) S.clfreq[S.cls[k]]++;
	}
	__syncthreads();
	huff_build(S.clfreq, 19, OP_PNG_CL_MAXBITS, S.cllens, S.clcodes, S.hw);
	// ---- sizes: this thread's bits, their prefix sum, and the block's form
	uint32_t mybits = 0;
	for (int k = 0; k < S.nsym[t]; ++k) {
		const uint32_t s = syms[t * PNG_SUB + k];
		if (s & 0x80000000u) {
			int c, eb, ev;
			len_code((int)((s >> 15) & 0x1FF), c, eb, ev); mybits += S.lens[c] + eb;
			dist_code((int)(s & 0x7FFF) + 1, c, eb, ev); mybits += S.lens[288 + c] + eb;
		} else mybits += S.lens[s];
	}
	S.bitoff[t] = mybits;
	__syncthreads();
	wg_scan_inclusive<256>(S.bitoff, t);
	if (t == 0) {
		int hclen = 19;
		while (hclen > 4 && !S.cllens[c_cl_order[hclen - 1]]) --hclen;
		S.hclen = hclen;
		uint32_t hb = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
		for (int k = 0; k < S.ncl; ++k) { const int c = S.cls[k]; hb += S.cllens[c] + (c == 16 ? 2 : c == 17 ? 3 : c == 18 ? 7 : 0); }
		S.hdr_bits = hb;
		const uint32_t bits = hb + S.bitoff[255] + S.lens[256];
		const uint32_t dyn_bytes = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
		const uint32_t stored_bytes = (uint32_t)L + 5;      // SEG <= 65535: one stored block
		S.use_stored = dyn_bytes >= stored_bytes;
		S.size = S.use_stored ? stored_bytes : dyn_bytes;
	}
	__syncthreads();
	if (S.use_stored) {
		if (t == 0) {
			slot[0] = last ? 1 : 0;
			slot[1] = (unsigned char)(L & 255); slot[2] = (unsigned char)(L >> 8);
			slot[3] = (unsigned char)(~L & 255); slot[4] = (unsigned char)((~L >> 8) & 255);
		}
		for (int j = t; j < L; j += 256) slot[5 + j] = F[s0 + j];
	} else {
		const int nwords = (int)((S.size + 3) / 4);
		for (int k = t; k < nwords; k += 256) S.u.outw[k] = 0;
		__syncthreads();
		LsbWriter bw;      // codec_shared.hpp; no put is longer than 16 bits
		if (t == 0) {
			bw.init(S.u.outw, 0);
			bw.put(last ? 1 : 0, 1); bw.put(2, 2);
			bw.put((uint32_t)(S.hlit - 257), 5); bw.put((uint32_t)(S.hdist - 1), 5); bw.put((uint32_t)(S.hclen - 4), 4);
			for (int k = 0; k < S.hclen; ++k) bw.put(S.cllens[c_cl_order[k]], 3);
			for (int k = 0; k < S.ncl; ++k) {
				const int c = S.cls[k];
				bw.put(S.clcodes[c], S.cllens[c]);
				if (c == 16) bw.put(S.clx[k], 2); else if (c == 17) bw.put(S.clx[k], 3); else if (c == 18) bw.put(S.clx[k], 7);
			}
			bw.flush();
		}
		bw.init(S.u.outw, S.hdr_bits + S.bitoff[t] - mybits);
		for (int k = 0; k < S.nsym[t]; ++k) {
			const uint32_t s = syms[t * PNG_SUB + k];
			if (s & 0x80000000u) {
				int c, eb, ev;
				len_code((int)((s >> 15) & 0x1FF), c, eb, ev); bw.put(S.codes[c], S.lens[c]); bw.put((uint32_t)ev, eb);
				dist_code((int)(s & 0x7FFF) + 1, c, eb, ev); bw.put(S.codes[288 + c], S.lens[288 + c]); bw.put((uint32_t)ev, eb);
			} else bw.put(S.codes[s], S.lens[s]);
		}
		bw.flush();
		if (t == 0) {
			const uint32_t end = S.hdr_bits + S.bitoff[255];
			bw.init(S.u.outw, end);
			bw.put(S.codes[256], S.lens[256]);
			bw.flush();
			if (!last) {      // empty stored block: 3 zero bits, zeros to the byte boundary, LEN = 0, NLEN = 0xFFFF
				const uint32_t q = (end + S.lens[256] + 3 + 7) / 8;
				bw.init(S.u.outw, 8 * (q + 2));
				bw.put(0xFFFFu, 16);
				bw.flush();
			}
		}
		__syncthreads();
		uint32_t* sw = reinterpret_cast<uint32_t*>(slot);
		for (int k = t; k < nwords; k += 256) sw[k] = S.u.outw[k];
	}
	if (t == 0) {
		sizes[seg] = S.size;
		adler_a[seg] = (uint32_t)(S.adA % PNG_ADLER);
		adler_b[seg] = (uint32_t)(S.adB % PNG_ADLER);
	}
}

// ------------------------------------------------ pack ------------------------------------------------
// GF(2) polynomials modulo the CRC-32 polynomial, reflected: bit 31 is x^0
__device__ uint32_t gf_mul(uint32_t a, uint32_t b) {
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}
__device__ uint32_t gf_xpow(unsigned long long e) {      // x^e
	uint32_t r = 1u << 31, base = 1u << 30;
	for (; e; e >>= 1) { if (e & 1) r = gf_mul(r, base); base = gf_mul(base, base); }
	return r;
}
__device__ __forceinline__ void put_be32(unsigned char* p, uint32_t v) { p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v; }
__device__ uint32_t crc_serial(const uint32_t* tab, const unsigned char* p, int n) {
	uint32_t c = 0xFFFFFFFFu;
	for (int i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255] ^ (c >> 8);
	return c ^ 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(256) k_png_pack(const unsigned char* __restrict__ slots, const uint32_t* __restrict__ sizes,
		const uint32_t* __restrict__ adler_a, const uint32_t* __restrict__ adler_b, long long N, int nseg, int h, int w,
		unsigned char* __restrict__ out, unsigned long long* __restrict__ total) {
	__shared__ uint32_t tab[256];
	__shared__ unsigned long long offs;
	__shared__ uint32_t crc;
	__shared__ unsigned char tmp[32];
	const int t = threadIdx.x, seg = blockIdx.x;
	{ uint32_t c = (uint32_t)t; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; tab[t] = c; }
	if (t == 0) { offs = 0; crc = 0; }
	wg_slot_offset(offs, sizes, seg, 12);      // a chunk is its data and 12 bytes: length, type, CRC
	const uint32_t size = sizes[seg];
	unsigned char* o = out + PNG_HEAD_BYTES + offs;
	const unsigned char* slot = slots + (long long)seg * PNG_SLOT;
	for (uint32_t j = t; j < size; j += 256) o[8 + j] = slot[j];
	// CRC-32 of "IDAT" + data, n bytes, by 256 threads: the message is right-aligned in 256 pieces of P bytes (zeros in front
	// leave a zero register unchanged), the initial value ~0 is folded into its first four bytes, piece t's register is
	// multiplied by x^(8 P (255 - t)) and the products are XORed
	{
		const uint32_t n = size + 4, P = (n + 255) / 256, pad = 256 * P - n;
		uint32_t c = 0;
		for (uint32_t v = (uint32_t)t * P; v < (uint32_t)(t + 1) * P; ++v) {
			if (v < pad) continue;
			const uint32_t m = v - pad;
			const uint32_t byte = m < 4 ? (uint32_t)("IDAT"[m] ^ 0xFF) & 255u : slot[m - 4];
			c = tab[(c ^ byte) & 255] ^ (c >> 8);
		}
		if (c) atomicXor(&crc, gf_mul(c, gf_xpow(8ull * P * (255 - t))));
	}
	__syncthreads();
	if (t == 0) {
		put_be32(o, size);
		o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
		put_be32(o + 8 + size, crc ^ 0xFFFFFFFFu);
	}
	if (seg == 0 && t == 0) {
		put_be32(out, 0x89504E47u); put_be32(out + 4, 0x0D0A1A0Au);      // the PNG signature
		tmp[0] = 'I'; tmp[1] = 'H'; tmp[2] = 'D'; tmp[3] = 'R';
		put_be32(tmp + 4, (uint32_t)w); put_be32(tmp + 8, (uint32_t)h);
		tmp[12] = 8; tmp[13] = 2; tmp[14] = 0; tmp[15] = 0; tmp[16] = 0;
		put_be32(out + 8, 13);
		for (int k = 0; k < 17; ++k) out[12 + k] = tmp[k];
		put_be32(out + 29, crc_serial(tab, tmp, 17));
		tmp[0] = 'I'; tmp[1] = 'D'; tmp[2] = 'A'; tmp[3] = 'T'; tmp[4] = 0x78; tmp[5] = 0x01;      // zlib header: deflate, 32 KiB window, fastest
		put_be32(out + 33, 2);
		for (int k = 0; k < 6; ++k) out[37 + k] = tmp[k];
		put_be32(out + 43, crc_serial(tab, tmp, 6));
	}
	if (seg == nseg - 1 && t == 0) {
		// Adler-32 of the whole filtered stream from the segments' (A = sum of bytes, B = sum of (L - j) * byte j)
		uint32_t s1 = 1, s2 = 0;
		for (int k = 0; k < nseg; ++k) {
			const unsigned long long len = (long long)(k + 1) * PNG_SEG < N ? PNG_SEG : N - (long long)k * PNG_SEG;
			s2 = (uint32_t)((s2 + len * s1 + adler_b[k]) % PNG_ADLER);
			s1 = (s1 + adler_a[k]) % PNG_ADLER;
		}
		unsigned char* e = o + 12 + size;
		tmp[0] = 'I'; tmp[1] = 'D'; tmp[2] = 'A'; tmp[3] = 'T';
		put_be32(tmp + 4, s2 << 16 | s1);
		put_be32(e, 4);
		for (int k = 0; k < 8; ++k) e[4 + k] = tmp[k];
		put_be32(e + 12, crc_serial(tab, tmp, 8));
		put_be32(e + 16, 0);
		e[20] = 'I'; e[21] = 'E'; e[22] = 'N'; e[23] = 'D';
		put_be32(e + 24, 0xAE426082u);
		*total = (unsigned long long)(e + 28 - out);
	}
}

// src: device H x W x 3, fp32 canvas or bytes; own: the call's blocks (on ctx->stream)
int encode_device(op_ctx* ctx, CallBlocks& own, const void* src, bool is_float, int h, int w, op_png** out, const char* who) {
	const long long N = (long long)h * (1 + 3LL * w);
	if (N > (1LL << 32)) OP_FAIL(OP_ERR_UNSUPPORTED, std::string(who) + ": filtered stream above 4 GiB");
	const int nseg = (int)((N + PNG_SEG - 1) / PNG_SEG);
	const size_t cap = (size_t)PNG_HEAD_BYTES + (size_t)N + (size_t)nseg * (12 + 5) + 16 + 12;
	hipStream_t st = ctx->stream;
	unsigned char *F = nullptr, *slots = nullptr, *obuf = nullptr; uint16_t* cand = nullptr; uint32_t *syms = nullptr, *meta = nullptr;
	unsigned long long* total = nullptr;
	HIPCHK(own.alloc(&F, (size_t)N));
	HIPCHK(own.alloc(&cand, sizeof(uint16_t) * (size_t)nseg * PNG_SEG));
	HIPCHK(own.alloc(&syms, sizeof(uint32_t) * (size_t)nseg * PNG_SEG));
	HIPCHK(own.alloc(&slots, (size_t)nseg * PNG_SLOT));
	HIPCHK(own.alloc(&meta, sizeof(uint32_t) * 3 * (size_t)nseg));
	HIPCHK(own.alloc(&obuf, cap));
	HIPCHK(own.alloc(&total, sizeof(unsigned long long)));
	uint32_t *sizes = meta, *ad_a = meta + nseg, *ad_b = meta + 2 * (size_t)nseg;
	HIPCHK(hipFuncSetAttribute((const void*)k_png_deflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(DeflateLds)));   // idempotent
	{ ProfScope ps(ctx, "png filter");
	  if (is_float) hipLaunchKernelGGL(k_png_filter<float>, dim3(h), dim3(256), 0, st, (const float*)src, h, w, F);
	  else hipLaunchKernelGGL(k_png_filter<unsigned char>, dim3(h), dim3(256), 0, st, (const unsigned char*)src, h, w, F);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "png deflate");
	  hipLaunchKernelGGL(k_png_deflate, dim3(nseg), dim3(256), sizeof(DeflateLds), st, F, N, nseg, cand, syms, slots, sizes, ad_a, ad_b);
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "png pack");
	  hipLaunchKernelGGL(k_png_pack, dim3(nseg), dim3(256), 0, st, slots, sizes, ad_a, ad_b, N, nseg, h, w, obuf, total);
	  HIPCHK(hipGetLastError()); }
	std::unique_ptr<op_png> png(new op_png);
	if (const int r = encoded_fetch(ctx, own, obuf, total, PNG_HEAD_BYTES, cap, *png, "png D2H", who)) return r;
	*out = png.release();
	return OP_OK;
}

}	// namespace

extern "C" {

int op_canvas_encode_png(op_ctx* ctx, const op_canvas* c, op_png** out) {
	if (!ctx || !c || !out) OP_FAIL(OP_ERR_INVALID, "op_canvas_encode_png: bad argument");
	int h = 0, w = 0;
	if (op_canvas_dims(c, &h, &w) != OP_OK) return OP_ERR_INVALID;
	if (h < 1 || w < 1) OP_FAIL(OP_ERR_INVALID, "op_canvas_encode_png: empty canvas (h = 0 or w = 0): a PNG cannot hold a zero-sized image");
	HIPCHK(hipSetDevice(ctx->device));
	CallBlocks own({ctx->stream});
	return encode_device(ctx, own, op_canvas_device(c), true, h, w, out, "op_canvas_encode_png");
}

int op_png_encode_u8(op_ctx* ctx, const unsigned char* rgb_host, int h, int w, op_png** out) {
	if (!ctx || !rgb_host || !out) OP_FAIL(OP_ERR_INVALID, "op_png_encode_u8: bad argument");
	if (h < 1 || w < 1) OP_FAIL(OP_ERR_INVALID, "op_png_encode_u8: empty image (h = 0 or w = 0): a PNG cannot hold a zero-sized image");
	HIPCHK(hipSetDevice(ctx->device));
	CallBlocks own({ctx->stream});
	unsigned char* d = nullptr;
	if (const int r = stage_rgb_u8(ctx, own, rgb_host, h, w, &d)) return r;
	return encode_device(ctx, own, d, false, h, w, out, "op_png_encode_u8");
}

int64_t op_png_size(const op_png* p) { return encoded_size(p); }
int op_png_copy(op_ctx*, const op_png* p, unsigned char* host) { return encoded_copy("op_png_copy", p, host); }

void op_png_free(op_png* p) { delete p; }

}	// extern "C"
