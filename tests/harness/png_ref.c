/* tests/harness/png_ref.c -- serial restatement of the device PNG encoder (openpano_amd/csrc/png.hip).
 *
 * Same filter choice, segment size, parse rule, Huffman construction and tie-breaks, written as one plain loop per stage:
 * the GPU tests require the device's file to equal this one byte for byte, the CPU tests decode this one with zlib.
 *
 *   filter    per scanline the PNG filter type (0..4, bpp 3) with the smallest sum of |residual as a signed byte|, ties to
 *             the lowest type.
 *   segments  the filtered stream (h * (1 + 3w) bytes) in pieces of SEG = 61440 bytes; every piece is its own IDAT chunk:
 *             one dynamic-Huffman block closed by an empty stored block (the last piece: BFINAL instead), or stored
 *             blocks when those are not larger.  The zlib header and the Adler-32 are IDAT chunks of their own.
 *   parse     every SUB = 240 bytes of a piece are parsed greedily on their own (a match never crosses a multiple of SUB
 *             counted from the piece's start).  Candidates at position i: distance 1, distance 3, and the hash candidate --
 *             the LATEST position with the same 13-bit hash of 3 bytes that lies in the 32768 bytes before the piece or
 *             in an EARLIER group of 256 positions of the piece (positions of i's own group are not candidates), if no
 *             farther than 32768.  The longest wins, then the nearest.  A match of length 3 farther than 4096 is dropped.
 *   Huffman   symbols ranked by (count, symbol); Moffat-Katajainen code lengths; Kraft fix-up to the limit (15, 7 for the
 *             code-length alphabet; the OP_PNG_*_MAXBITS knobs of png.hip); lengths dealt shortest-first to the highest
 *             rank; canonical codes.
 *
 * png_ref_stats reports what the last png_ref_encode went through (which limiter fired, the longest codes, the codes used):
 * counters only, no byte of the file depends on them.  The tests assert every "this input reaches X" claim from them.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SEG 61440   /* 256 sub-blocks; a multiple of 3, so that 2 SEG + 1 is a possible stream length */
#define SUB 240
#define WINDOW 32768
#define HASH_BITS 13
#define TOO_FAR 4096
#define ADLER_MOD 65521u

/* the same three knobs as png.hip: RFC 1951 bounds code lengths from above only, so a tighter limit still gives a valid file */
#ifndef OP_PNG_LIT_MAXBITS
#define OP_PNG_LIT_MAXBITS 15
#endif
#ifndef OP_PNG_DIST_MAXBITS
#define OP_PNG_DIST_MAXBITS 15
#endif
#ifndef OP_PNG_CL_MAXBITS
#define OP_PNG_CL_MAXBITS 7
#endif
_Static_assert(OP_PNG_LIT_MAXBITS >= 9 && OP_PNG_LIT_MAXBITS <= 15, "286 codes need 9 bits; deflate allows 15");
_Static_assert(OP_PNG_DIST_MAXBITS >= 5 && OP_PNG_DIST_MAXBITS <= 15, "30 codes need 5 bits; deflate allows 15");
_Static_assert(OP_PNG_CL_MAXBITS >= 5 && OP_PNG_CL_MAXBITS <= 7, "19 codes need 5 bits; a code-length code length is a 3-bit field");

/* what the last png_ref_encode went through; index 0 literal / length, 1 distance, 2 code-length alphabet */
typedef struct {
	int32_t limited[3];          /* segments in which the Kraft fix-up changed the tree (stored segments included) */
	int32_t limited_dynamic[3];  /* ... of them written as a dynamic block, i.e. the limited table is in the file */
	int32_t depth[3];            /* longest code length before the limit */
	int32_t maxlen[3];           /* longest code length after it */
	int32_t stored, dynamic;     /* segments of either form */
	uint32_t len_codes;          /* bit c: length code 257 + c, distance code c, code-length symbol c used in a dynamic segment */
	uint32_t dist_codes;
	uint32_t cl_syms;
	int32_t limited_not_last;    /* a dynamic segment with a limited table that is not the last one */
	int32_t maxbits[3];          /* the limits this library was compiled with */
} png_ref_stats_t;
static png_ref_stats_t g_stats;

static uint32_t crc_table[256];
static void crc_init(void) {
	for (uint32_t n = 0; n < 256; ++n) {
		uint32_t c = n;
		for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
		crc_table[n] = c;
	}
}
static uint32_t crc32_of(const unsigned char* p, size_t n) {
	uint32_t c = 0xFFFFFFFFu;
	for (size_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 255] ^ (c >> 8);
	return c ^ 0xFFFFFFFFu;
}
static void be32(unsigned char* p, uint32_t v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }

/* one chunk: length, type, data, CRC over type + data; returns the bytes written */
static size_t put_chunk(unsigned char* out, const char* type, const unsigned char* data, uint32_t n) {
	be32(out, n);
	memcpy(out + 4, type, 4);
	if (n) memcpy(out + 8, data, n);
	be32(out + 8 + n, crc32_of(out + 4, 4 + (size_t)n));
	return 12 + (size_t)n;
}

/* ---- filter ---- */
static int paeth(int a, int b, int c) {
	const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
	return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
static unsigned char filt(int type, int cur, int a, int b, int c) {
	switch (type) {
	case 0: return (unsigned char)cur;
	case 1: return (unsigned char)(cur - a);
	case 2: return (unsigned char)(cur - b);
	case 3: return (unsigned char)(cur - ((a + b) >> 1));
	default: return (unsigned char)(cur - paeth(a, b, c));
	}
}
static void filter_image(const unsigned char* rgb, int h, int w, unsigned char* F) {
	const long R = 3L * w;
	for (int y = 0; y < h; ++y) {
		const unsigned char* cur = rgb + (long)y * R;
		const unsigned char* up = y ? cur - R : NULL;
		long sum[5] = {0, 0, 0, 0, 0};
		for (long x = 0; x < R; ++x) {
			const int a = x >= 3 ? cur[x - 3] : 0, b = up ? up[x] : 0, c = (up && x >= 3) ? up[x - 3] : 0;
			for (int t = 0; t < 5; ++t) { const int v = filt(t, cur[x], a, b, c); sum[t] += v < 128 ? v : 256 - v; }
		}
		int best = 0;
		for (int t = 1; t < 5; ++t) if (sum[t] < sum[best]) best = t;
		unsigned char* o = F + (long)y * (R + 1);
		o[0] = (unsigned char)best;
		for (long x = 0; x < R; ++x) {
			const int a = x >= 3 ? cur[x - 3] : 0, b = up ? up[x] : 0, c = (up && x >= 3) ? up[x - 3] : 0;
			o[1 + x] = filt(best, cur[x], a, b, c);
		}
	}
}

/* ---- bit writer, LSB first ---- */
typedef struct { unsigned char* p; uint64_t nbits; } bitw;
static void put_bits(bitw* b, uint32_t v, int n) {
	for (int k = 0; k < n; ++k, ++b->nbits) if ((v >> k) & 1) b->p[b->nbits >> 3] |= (unsigned char)(1u << (b->nbits & 7));
}

/* ---- Huffman ---- */
/* info (counters only): [0] the fix-up loop ran, [1] longest length before the limit, [2] after it */
static void huff_build(const uint32_t* freq, int n, int maxbits, unsigned char* lens, uint16_t* codes, int* info) {
	uint32_t key[288]; int sym[288]; int num[33]; uint32_t next_code[17];
	int used = 0;
	info[0] = info[1] = info[2] = 0;
	memset(lens, 0, (size_t)n);
	memset(codes, 0, sizeof(uint16_t) * (size_t)n);
	/* rank by (count, symbol) */
	for (int s = 0; s < n; ++s) {
		if (!freq[s]) continue;
		int r = 0;
		for (int q = 0; q < n; ++q) if (freq[q] && (freq[q] < freq[s] || (freq[q] == freq[s] && q < s))) ++r;
		key[r] = freq[s]; sym[r] = s; ++used;
	}
	if (used == 0) return;
	if (used == 1) key[0] = 1;
	else {
		/* Moffat & Katajainen, in-place minimum-redundancy code lengths */
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
	/* limit the lengths: counts per length, Kraft fix-up */
	memset(num, 0, sizeof(num));
	for (int i = 0; i < used; ++i) num[key[i] > 32 ? 32 : key[i]]++;
	for (int i = 1; i <= 32; ++i) if (num[i]) info[1] = i;
	if (used > 1) {
		uint32_t total = 0;
		for (int i = maxbits + 1; i <= 32; ++i) { num[maxbits] += num[i]; num[i] = 0; }
		for (int i = maxbits; i > 0; --i) total += (uint32_t)num[i] << (maxbits - i);
		while (total != (1u << maxbits)) {
			num[maxbits]--;
			for (int i = maxbits - 1; i > 0; --i) if (num[i]) { num[i]--; num[i + 1] += 2; break; }
			--total;
			info[0] = 1;
		}
	}
	for (int i = 1; i <= maxbits; ++i) if (num[i]) info[2] = i;
	/* shortest lengths to the highest ranks */
	for (int i = 1, j = used; i <= maxbits; ++i) for (int l = num[i]; l > 0; --l) lens[sym[--j]] = (unsigned char)i;
	/* canonical codes, stored bit-reversed (deflate packs Huffman codes MSB first into an LSB-first stream) */
	{
		uint32_t code = 0;
		next_code[0] = 0;
		for (int b = 1; b <= maxbits; ++b) { code = (code + (b > 1 ? (uint32_t)num[b - 1] : 0)) << 1; next_code[b] = code; }
		for (int s = 0; s < n; ++s) {
			if (!lens[s]) continue;
			uint32_t c = next_code[lens[s]]++, r = 0;
			for (int b = 0; b < lens[s]; ++b) r |= ((c >> b) & 1) << (lens[s] - 1 - b);
			codes[s] = (uint16_t)r;
		}
	}
}

static int ilog2(uint32_t v) { int n = 0; while (v >>= 1) ++n; return n; }
static void len_code(int len, int* code, int* ebits, int* eval) {
	const int l = len - 3;
	if (len == 258) { *code = 285; *ebits = 0; *eval = 0; }
	else if (l < 8) { *code = 257 + l; *ebits = 0; *eval = 0; }
	else { const int e = ilog2((uint32_t)l) - 2; *code = 257 + 4 * (e + 1) + ((l >> e) & 3); *ebits = e; *eval = l & ((1 << e) - 1); }
}
static void dist_code(int dist, int* code, int* ebits, int* eval) {
	const int d = dist - 1;
	if (d < 4) { *code = d; *ebits = 0; *eval = 0; }
	else { const int e = ilog2((uint32_t)d) - 1; *code = 2 * (e + 1) + ((d >> e) & 1); *ebits = e; *eval = d & ((1 << e) - 1); }
}

static uint32_t hash3(const unsigned char* p) {
	return (((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16) * 2654435761u) >> (32 - HASH_BITS);
}
static int match_len(const unsigned char* F, long i, long d, int maxlen) {
	int k = 0;
	while (k < maxlen && F[i + k] == F[i - d + k]) ++k;
	return k;
}

static const unsigned char cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

/* one segment [s0, s1) of the filtered stream F (N bytes) -> deflate bytes at out (zeroed, SEG + 16 bytes); returns their count */
static long encode_segment(const unsigned char* F, long N, long s0, long s1, int last, unsigned char* out) {
	const long L = s1 - s0;
	static int32_t head[1 << HASH_BITS];
	static uint16_t cand[SEG];
	static uint32_t syms[SEG];
	static int nsym[SEG / SUB];
	const int nsub = (int)((L + SUB - 1) / SUB);
	/* hash candidates: positions are kept as (p - s0 + WINDOW + 1), 0 = empty */
	memset(head, 0, sizeof(head));
	for (long p = s0 - WINDOW < 0 ? 0 : s0 - WINDOW; p < s0; ++p) if (p + 2 < N) head[hash3(F + p)] = (int32_t)(p - s0 + WINDOW + 1);
	for (long g = 0; g < L; g += 256) {
		const long ge = g + 256 < L ? g + 256 : L;
		for (long q = g; q < ge; ++q) {
			const long p = s0 + q;
			cand[q] = 0;
			if (p + 2 < N) {
				const int32_t hd = head[hash3(F + p)];
				if (hd) { const long d = (q + WINDOW + 1) - hd; if (d <= WINDOW) cand[q] = (uint16_t)d; }
			}
		}
		for (long q = g; q < ge; ++q) if (s0 + q + 2 < N) head[hash3(F + s0 + q)] = (int32_t)(q + WINDOW + 1);
	}
	/* greedy parse of every sub-block */
	uint32_t freq[320];
	memset(freq, 0, sizeof(freq));
	for (int t = 0; t < nsub; ++t) {
		long i = s0 + (long)t * SUB;
		const long e = i + SUB < s1 ? i + SUB : s1;
		int n = 0;
		while (i < e) {
			const int maxlen = e - i < 258 ? (int)(e - i) : 258;
			const long ds[3] = {1, 3, cand[i - s0]};
			int bl = 0; long bd = 0;
			for (int k = 0; k < 3; ++k) {
				const long d = ds[k];
				if (d == 0 || d > i) continue;
				const int l = match_len(F, i, d, maxlen);
				if (l > bl || (l == bl && l > 0 && d < bd)) { bl = l; bd = d; }
			}
			if (bl >= 3 && !(bl == 3 && bd > TOO_FAR)) {
				int c, eb, ev;
				syms[t * SUB + n++] = 0x80000000u | (uint32_t)bl << 15 | (uint32_t)(bd - 1);
				len_code(bl, &c, &eb, &ev); freq[c]++;
				dist_code((int)bd, &c, &eb, &ev); freq[288 + c]++;
				i += bl;
			} else { syms[t * SUB + n++] = F[i]; freq[F[i]]++; ++i; }
		}
		nsym[t] = n;
	}
	uint32_t dist_used = 0;
	for (int c = 0; c < 30; ++c) if (freq[288 + c]) dist_used |= 1u << c;      /* before the stand-in code of a match-free segment */
	freq[256] = 1;
	{ int any = 0; for (int c = 0; c < 30; ++c) any |= freq[288 + c] != 0; if (!any) freq[288] = 1; }
	unsigned char lens[320]; uint16_t codes[320];
	int info[3][3];
	huff_build(freq, 286, OP_PNG_LIT_MAXBITS, lens, codes, info[0]);
	huff_build(freq + 288, 30, OP_PNG_DIST_MAXBITS, lens + 288, codes + 288, info[1]);
	int hlit = 286, hdist = 30;
	while (hlit > 257 && !lens[hlit - 1]) --hlit;
	while (hdist > 1 && !lens[288 + hdist - 1]) --hdist;
	/* code lengths of both alphabets as one sequence, run-length coded with 16 / 17 / 18 */
	unsigned char seq[316]; unsigned char cls[316], clx[316]; int ncl = 0, nseq = 0;
	for (int k = 0; k < hlit; ++k) seq[nseq++] = lens[k];
	for (int k = 0; k < hdist; ++k) seq[nseq++] = lens[288 + k];
	for (int k = 0; k < nseq;) {
		int r = 1;
		while (k + r < nseq && seq[k + r] == seq[k]) ++r;
		const int v = seq[k];
		k += r;
		if (v == 0) {
			while (r >= 11) { const int m = r < 138 ? r : 138; cls[ncl] = 18; clx[ncl++] = (unsigned char)(m - 11); r -= m; }
			if (r >= 3) { cls[ncl] = 17; clx[ncl++] = (unsigned char)(r - 3); r = 0; }
			while (r-- > 0) { cls[ncl] = 0; clx[ncl++] = 0; }
		} else {
			cls[ncl] = (unsigned char)v; clx[ncl++] = 0; --r;
			while (r >= 3) { const int m = r < 6 ? r : 6; cls[ncl] = 16; clx[ncl++] = (unsigned char)(m - 3); r -= m; }
			while (r-- > 0) { cls[ncl] = (unsigned char)v; clx[ncl++] = 0; }
		}
	}
	uint32_t clfreq[19]; unsigned char cllens[19]; uint16_t clcodes[19];
	memset(clfreq, 0, sizeof(clfreq));
	for (int k = 0; k < ncl; ++k) clfreq[cls[k]]++;
	huff_build(clfreq, 19, OP_PNG_CL_MAXBITS, cllens, clcodes, info[2]);
	int hclen = 19;
	while (hclen > 4 && !cllens[cl_order[hclen - 1]]) --hclen;
	/* sizes: dynamic block (+ the empty stored block that byte-aligns every segment but the last) against stored blocks */
	uint64_t bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
	for (int k = 0; k < ncl; ++k) bits += cllens[cls[k]] + (cls[k] == 16 ? 2 : cls[k] == 17 ? 3 : cls[k] == 18 ? 7 : 0);
	for (int t = 0; t < nsub; ++t) for (int k = 0; k < nsym[t]; ++k) {
		const uint32_t s = syms[t * SUB + k];
		if (s & 0x80000000u) {
			int c, eb, ev;
			len_code((int)((s >> 15) & 0x1FF), &c, &eb, &ev); bits += lens[c] + eb;
			dist_code((int)(s & 0x7FFF) + 1, &c, &eb, &ev); bits += lens[288 + c] + eb;
		} else bits += lens[s];
	}
	bits += lens[256];
	const long dyn_bytes = last ? (long)((bits + 7) / 8) : (long)((bits + 3 + 7) / 8) + 4;
	const long nstored = (L + 65534) / 65535;
	const long stored_bytes = L + 5 * nstored;
	const int dynamic = dyn_bytes < stored_bytes;
	for (int a = 0; a < 3; ++a) {
		g_stats.limited[a] += info[a][0];
		if (dynamic) g_stats.limited_dynamic[a] += info[a][0];
		if (info[a][1] > g_stats.depth[a]) g_stats.depth[a] = info[a][1];
		if (info[a][2] > g_stats.maxlen[a]) g_stats.maxlen[a] = info[a][2];
	}
	if (dynamic) {
		++g_stats.dynamic;
		for (int c = 257; c < 286; ++c) if (freq[c]) g_stats.len_codes |= 1u << (c - 257);
		g_stats.dist_codes |= dist_used;
		for (int c = 0; c < 19; ++c) if (clfreq[c]) g_stats.cl_syms |= 1u << c;
		if (!last && (info[0][0] || info[1][0] || info[2][0])) g_stats.limited_not_last = 1;
	} else ++g_stats.stored;
	if (!dynamic) {
		long o = 0;
		for (long b = 0; b < nstored; ++b) {
			const long off = b * 65535, n = L - off < 65535 ? L - off : 65535;
			out[o++] = (unsigned char)((last && b == nstored - 1) ? 1 : 0);
			out[o++] = (unsigned char)(n & 255); out[o++] = (unsigned char)(n >> 8);
			out[o++] = (unsigned char)(~n & 255); out[o++] = (unsigned char)((~n >> 8) & 255);
			memcpy(out + o, F + s0 + off, (size_t)n); o += n;
		}
		return o;
	}
	bitw bw = {out, 0};
	put_bits(&bw, last ? 1 : 0, 1); put_bits(&bw, 2, 2);
	put_bits(&bw, (uint32_t)(hlit - 257), 5); put_bits(&bw, (uint32_t)(hdist - 1), 5); put_bits(&bw, (uint32_t)(hclen - 4), 4);
	for (int k = 0; k < hclen; ++k) put_bits(&bw, cllens[cl_order[k]], 3);
	for (int k = 0; k < ncl; ++k) {
		put_bits(&bw, clcodes[cls[k]], cllens[cls[k]]);
		if (cls[k] == 16) put_bits(&bw, clx[k], 2); else if (cls[k] == 17) put_bits(&bw, clx[k], 3); else if (cls[k] == 18) put_bits(&bw, clx[k], 7);
	}
	for (int t = 0; t < nsub; ++t) for (int k = 0; k < nsym[t]; ++k) {
		const uint32_t s = syms[t * SUB + k];
		if (s & 0x80000000u) {
			int c, eb, ev;
			len_code((int)((s >> 15) & 0x1FF), &c, &eb, &ev); put_bits(&bw, codes[c], lens[c]); put_bits(&bw, (uint32_t)ev, eb);
			dist_code((int)(s & 0x7FFF) + 1, &c, &eb, &ev); put_bits(&bw, codes[288 + c], lens[288 + c]); put_bits(&bw, (uint32_t)ev, eb);
		} else put_bits(&bw, codes[s], lens[s]);
	}
	put_bits(&bw, codes[256], lens[256]);
	if (!last) {
		put_bits(&bw, 0, 3);
		bw.nbits = (bw.nbits + 7) & ~(uint64_t)7;
		put_bits(&bw, 0, 16); put_bits(&bw, 0xFFFF, 16);
	}
	return (long)((bw.nbits + 7) / 8);
}

/* upper bound of the file's size (what png_ref_encode needs as capacity) */
long png_ref_bound(int h, int w) {
	const long N = (long)h * (1 + 3L * w), nseg = (N + SEG - 1) / SEG;
	return 8 + 25 + 14 + 16 + 12 + N + nseg * (12 + 5);
}
long png_ref_segment(void) { return SEG; }
/* the statistics of the last png_ref_encode */
void png_ref_stats(png_ref_stats_t* out) { *out = g_stats; }

/* H x W x 3 bytes -> the PNG file; returns its size, -1 on bad arguments / too little room */
long png_ref_encode(const unsigned char* rgb, int h, int w, unsigned char* out, long cap) {
	if (!rgb || !out || h < 1 || w < 1 || cap < png_ref_bound(h, w)) return -1;
	crc_init();
	memset(&g_stats, 0, sizeof(g_stats));
	g_stats.maxbits[0] = OP_PNG_LIT_MAXBITS; g_stats.maxbits[1] = OP_PNG_DIST_MAXBITS; g_stats.maxbits[2] = OP_PNG_CL_MAXBITS;
	const long N = (long)h * (1 + 3L * w), nseg = (N + SEG - 1) / SEG;
	unsigned char* F = (unsigned char*)malloc((size_t)N + 4);
	unsigned char* slot = (unsigned char*)malloc(SEG + 16);
	if (!F || !slot) { free(F); free(slot); return -1; }
	filter_image(rgb, h, w, F);
	static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
	long o = 0;
	memcpy(out, sig, 8); o = 8;
	unsigned char ihdr[13];
	be32(ihdr, (uint32_t)w); be32(ihdr + 4, (uint32_t)h);
	ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
	o += (long)put_chunk(out + o, "IHDR", ihdr, 13);
	const unsigned char zhdr[2] = {0x78, 0x01};
	o += (long)put_chunk(out + o, "IDAT", zhdr, 2);
	uint32_t s1 = 1, s2 = 0;
	for (long k = 0; k < nseg; ++k) {
		const long a = k * SEG, b = a + SEG < N ? a + SEG : N;
		memset(slot, 0, SEG + 16);
		const long n = encode_segment(F, N, a, b, k == nseg - 1, slot);
		o += (long)put_chunk(out + o, "IDAT", slot, (uint32_t)n);
		/* Adler-32 from the segment's partial sums: A = sum of bytes, B = sum of (L - j) * byte j */
		uint64_t A = 0, B = 0;
		for (long j = a; j < b; ++j) { A += F[j]; B += (uint64_t)(b - j) * F[j]; }
		s2 = (uint32_t)((s2 + (uint64_t)(b - a) * s1 + B) % ADLER_MOD);
		s1 = (uint32_t)((s1 + A) % ADLER_MOD);
	}
	unsigned char ad[4];
	be32(ad, s2 << 16 | s1);
	o += (long)put_chunk(out + o, "IDAT", ad, 4);
	o += (long)put_chunk(out + o, "IEND", NULL, 0);
	free(F); free(slot);
	return o;
}
