/* jpeg_dec_ref.c -- the serial restatement of openpano_amd/csrc/jpeg_dec.hip: a baseline JPEG decoder
 * as plain loops.  One sequential Huffman decode per restart interval, no subsequences, no synchronisation; integer
 * arithmetic only.  Its pixels are compared byte for byte with libjpeg's (tests/test_jpeg_dec_cpu.py, where Pillow imports) and
 * with the device's (tests/test_gpu_jpeg_dec.py).  jpeg_dec_ref_stats says what the last decode went through, and
 * jpeg_dec_ref_trace gives the decoder's state at every subsequence boundary, which the synchronisation must reach. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
	int32_t stuffed, zrl, end63, max_dc_cat, max_ac_cat, max_code_len, intervals, blocks;
	int32_t max_zrl_chain;            /* the longest run of ZRL symbols in a row */
	int32_t unpadded, unpadded_last, pad_zero;     /* intervals that end on a byte boundary; whether the last one does; intervals with a 0 among their pad bits */
	int32_t end_ff;                   /* intervals whose last data byte is FF */
	int32_t eob_after_dc, full_blocks, run15;      /* blocks of a DC and an EOB; blocks of 63 non-zero ACs; symbols F1..FA */
	int32_t end63_zrl[4];             /* coefficient 63 written right behind 0, 1, 2, 3 ZRLs */
	int32_t dc_bound[12], ac_bound[11];            /* per category s: bit 0: -(2^s - 1) seen, 1: -2^(s-1), 2: +2^(s-1), 3: +(2^s - 1) */
} jpeg_dec_ref_stats_t;
static jpeg_dec_ref_stats_t g_stats;
void jpeg_dec_ref_stats(jpeg_dec_ref_stats_t* s) { *s = g_stats; }

static const uint8_t ZZ[64] = {
	0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
	35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

typedef struct { int count[17]; int first[17]; int at[17]; uint8_t vals[256]; int defined; } huff_t;
typedef struct {
	int h, w, ncomp, hs, vs, ri;
	int tq[3], td[3], ta[3];
	int q[4][64], have_q[4];          /* zigzag order, as in the file */
	huff_t dc[4], ac[4];
	long scan;                        /* first byte of the entropy-coded data */
} frame_t;

static int be16(const uint8_t* p) { return p[0] << 8 | p[1]; }

/* 0, or -1 (broken) / -4 (outside the format) */
static int parse(const uint8_t* f, long size, frame_t* F) {
	memset(F, 0, sizeof *F);
	F->hs = F->vs = 1;
	if (size < 4 || f[0] != 0xFF || f[1] != 0xD8) return -1;
	long pos = 2;
	int sof = 0;
	for (;;) {
		if (pos + 4 > size || f[pos] != 0xFF) return -1;
		const int m = f[pos + 1];
		if (m == 0xFF) { ++pos; continue; }
		const long L = be16(f + pos + 2);
		if (L < 2 || pos + 2 + L > size) return -1;
		const uint8_t* p = f + pos + 4;
		if (m == 0xC0) {
			if (p[0] != 8) return -4;
			F->h = be16(p + 1); F->w = be16(p + 3); F->ncomp = p[5];
			if (F->ncomp != 1 && F->ncomp != 3) return -4;
			if (L != 8 + 3 * F->ncomp) return -1;
			for (int c = 0; c < F->ncomp; ++c) {
				const int s = p[7 + 3 * c];
				F->tq[c] = p[8 + 3 * c] & 3;
				if (c == 0 && F->ncomp == 3) {
					if (s != 0x11 && s != 0x21 && s != 0x22) return -4;
					F->hs = s >> 4; F->vs = s & 15;
				} else if (s != 0x11) return -4;
			}
			sof = 1;
		} else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) return -4;
		else if (m == 0xC4) {
			long o = 0;
			while (o + 17 <= L - 2) {
				huff_t* t = (p[o] >> 4) ? &F->ac[p[o] & 3] : &F->dc[p[o] & 3];
				int n = 0, code = 0;
				for (int len = 1; len <= 16; ++len) {
					t->count[len] = p[o + len]; t->first[len] = code; t->at[len] = n;
					n += t->count[len]; code = (code + t->count[len]) << 1;
				}
				if (n > 256 || o + 17 + n > L - 2) return -1;
				memcpy(t->vals, p + o + 17, (size_t)n);
				t->defined = 1;
				o += 17 + n;
			}
		} else if (m == 0xDB) {
			for (long o = 0; o + 65 <= L - 2; o += 65) {
				if (p[o] >> 4) return -4;
				for (int k = 0; k < 64; ++k) F->q[p[o] & 3][k] = p[o + 1 + k];
				F->have_q[p[o] & 3] = 1;
			}
		} else if (m == 0xDD) F->ri = be16(p);
		else if (m == 0xDA) {
			if (!sof || p[0] != F->ncomp) return -4;
			for (int c = 0; c < F->ncomp; ++c) { F->td[c] = (p[2 + 2 * c] >> 4) & 3; F->ta[c] = p[2 + 2 * c] & 3; }
			F->scan = pos + 2 + L;
			break;
		}
		pos += 2 + L;
	}
	for (int c = 0; c < F->ncomp; ++c)
		if (!F->have_q[F->tq[c]] || !F->dc[F->td[c]].defined || !F->ac[F->ta[c]].defined) return -1;
	return F->h >= 1 && F->w >= 1 ? 0 : -1;
}

int jpeg_dec_ref_probe(const uint8_t* f, long size, int* h, int* w, int* sampling) {
	frame_t F;
	const int r = parse(f, size, &F);
	if (r) return r;
	*h = F.h; *w = F.w;
	*sampling = F.ncomp == 1 ? 3 : F.hs == 1 ? 0 : F.vs == 2 ? 1 : 2;
	return 0;
}

/* the entropy-coded data without stuffing and markers; iv[j]: first byte of interval j, iv[*nint]: the total.  -1: a stray marker */
static long unstuff(const uint8_t* f, long size, long pos, uint8_t* out, long* iv, long max_iv, long* nint) {
	long n = 0, k = 0;
	iv[0] = 0;
	for (;;) {
		if (pos >= size) return -1;
		if (f[pos] != 0xFF) { out[n++] = f[pos++]; continue; }
		if (pos + 1 >= size) return -1;
		const int m = f[pos + 1];
		if (m == 0) { out[n++] = 0xFF; pos += 2; ++g_stats.stuffed; }
		else if (m == 0xD9) break;
		else if (m == 0xD0 + (k & 7)) { if (k + 1 >= max_iv) return -1; iv[++k] = n; pos += 2; }
		else return -1;
	}
	iv[k + 1] = n;
	*nint = k + 1;
	return n;
}

typedef struct { const uint8_t* d; long pos, end; } bits_t;      /* positions in bits */
static int get_bit(bits_t* b) {
	if (b->pos >= b->end) { ++b->pos; return -1; }
	const int v = (b->d[b->pos >> 3] >> (7 - (b->pos & 7))) & 1;
	++b->pos;
	return v;
}
/* the next symbol: bit by bit along the canonical code; -1 when no code matches or the data ends */
static int get_symbol(bits_t* b, const huff_t* t) {
	int code = 0;
	for (int len = 1; len <= 16; ++len) {
		const int bit = get_bit(b);
		if (bit < 0) return -1;
		code = code << 1 | bit;
		if (code - t->first[len] < t->count[len] && code >= t->first[len]) {
			if (len > g_stats.max_code_len) g_stats.max_code_len = len;
			return t->vals[t->at[len] + code - t->first[len]];
		}
	}
	return -1;
}
static int get_value(bits_t* b, int s, int* bad) {
	int v = 0;
	for (int i = 0; i < s; ++i) { const int bit = get_bit(b); if (bit < 0) { *bad = 1; return 0; } v = v << 1 | bit; }
	return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

/* the boundary states of the subsequences of S bits, four words each: position, block in MCU, zigzag position (| 0x100 on an
 * interval's last subsequence), blocks completed */
typedef struct { uint32_t* out; long cap, n; long S, sub_end, iv_end; uint32_t done; int on; } trace_t;
static void trace_boundary(trace_t* T, long pos, int k, int zz) {
	while (T->on && pos >= T->sub_end && T->sub_end <= T->iv_end) {
		if (T->out && T->n < T->cap) { uint32_t* o = T->out + 4 * T->n; o[0] = (uint32_t)pos; o[1] = (uint32_t)k; o[2] = (uint32_t)zz | (T->sub_end == T->iv_end ? 0x100u : 0u); o[3] = T->done; }
		++T->n; T->done = 0;
		if (T->sub_end == T->iv_end) { T->sub_end = T->iv_end + 1; break; }
		T->sub_end = T->sub_end + T->S < T->iv_end ? T->sub_end + T->S : T->iv_end;
	}
}

static void note_bound(int32_t* seen, int s, int v) {
	if (v == -((1 << s) - 1)) seen[s] |= 1;
	if (v == -(1 << (s - 1))) seen[s] |= 2;
	if (v == 1 << (s - 1)) seen[s] |= 4;
	if (v == (1 << s) - 1) seen[s] |= 8;
}

/* one block: coefficients in natural order, the DC as the value (pred updated).  0, or -1 on broken data */
static int decode_block(bits_t* b, const huff_t* dc, const huff_t* ac, int* pred, int16_t* coef, trace_t* T, int kblk) {
	int bad = 0;
	int s = get_symbol(b, dc);
	if (s < 0 || s > 11) return -1;
	if (s > g_stats.max_dc_cat) g_stats.max_dc_cat = s;
	const int diff = get_value(b, s, &bad);
	if (bad) return -1;
	if (s) note_bound(g_stats.dc_bound, s, diff);
	*pred += diff;
	coef[0] = (int16_t)*pred;
	trace_boundary(T, b->pos, kblk, 1);
	int k = 1, chain = 0, nonzero = 0;
	while (k < 64) {
		const int rs = get_symbol(b, ac);
		if (rs < 0) return -1;
		const int r = rs >> 4;
		s = rs & 15;
		if (s == 0) {
			if (r != 15) { if (k == 1) ++g_stats.eob_after_dc; k = 64; break; }      /* EOB */
			if (k + 16 > 63) return -1;
			k += 16; ++g_stats.zrl;
			if (++chain > g_stats.max_zrl_chain) g_stats.max_zrl_chain = chain;
			trace_boundary(T, b->pos, kblk, k);
			continue;
		}
		if (s > 10) return -1;
		if (s > g_stats.max_ac_cat) g_stats.max_ac_cat = s;
		k += r;
		if (k > 63) return -1;
		coef[ZZ[k]] = (int16_t)get_value(b, s, &bad);
		if (bad) return -1;
		note_bound(g_stats.ac_bound, s, coef[ZZ[k]]);
		if (r == 15) ++g_stats.run15;
		if (k == 63) { ++g_stats.end63; if (chain < 4) ++g_stats.end63_zrl[chain]; }
		if (++nonzero == 63) ++g_stats.full_blocks;
		chain = 0;
		++k;
		if (k < 64) trace_boundary(T, b->pos, kblk, k);
	}
	return 0;
}

static int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
static int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

/* jpeg_idct_islow over d[0], d[stride], ..: pass 0 = columns (descale by 11), pass 1 = rows (descale by 18) */
static void idct_pass(int* d, int stride, int pass) {
	const int i0 = d[0], i1 = d[stride], i2 = d[2 * stride], i3 = d[3 * stride], i4 = d[4 * stride], i5 = d[5 * stride], i6 = d[6 * stride], i7 = d[7 * stride];
	const int sh = pass ? 18 : 11;
	int z1 = (i2 + i6) * 4433;
	const int tmp2 = z1 + i6 * -15137, tmp3 = z1 + i2 * 6270;
	const int tmp0 = (i0 + i4) * 8192, tmp1 = (i0 - i4) * 8192;
	const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
	int t0 = i7, t1 = i5, t2 = i3, t3 = i1;
	z1 = t0 + t3;
	int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
	const int z5 = (z3 + z4) * 9633;
	t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
	z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
	z3 += z5; z4 += z5;
	t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
	d[0] = descale(tmp10 + t3, sh); d[7 * stride] = descale(tmp10 - t3, sh);
	d[stride] = descale(tmp11 + t2, sh); d[6 * stride] = descale(tmp11 - t2, sh);
	d[2 * stride] = descale(tmp12 + t1, sh); d[5 * stride] = descale(tmp12 - t1, sh);
	d[3 * stride] = descale(tmp13 + t0, sh); d[4 * stride] = descale(tmp13 - t0, sh);
}

/* chroma for output pixel (y, x): libjpeg's h2v1 / h2v2 fancy upsampling where the downsampled width exceeds 2, replication otherwise */
static int chroma(const uint8_t* p, int pitch, int cw, int ch, int hs, int vs, int y, int x) {
	if (hs == 1) return p[(long)y * pitch + x];
	const int c = x / 2;
	if (vs == 1) {
		const uint8_t* in = p + (long)y * pitch;
		if (cw <= 2) return in[c];
		if (x % 2 == 0) return c == 0 ? in[0] : (3 * in[c] + in[c - 1] + 1) >> 2;
		return c == cw - 1 ? in[c] : (3 * in[c] + in[c + 1] + 2) >> 2;
	}
	const int r = y / 2;
	if (cw <= 2) return p[(long)r * pitch + c];
	int far = y % 2 ? r + 1 : r - 1;      /* row -1 is row 0; below the last real row, that row again */
	if (far < 0) far = 0;
	if (far > ch - 1) far = ch - 1;
	const uint8_t* near_row = p + (long)r * pitch; const uint8_t* far_row = p + (long)far * pitch;
	const int cur = 3 * near_row[c] + far_row[c];
	if (x % 2 == 0) return c == 0 ? (4 * cur + 8) >> 4 : (3 * cur + (3 * near_row[c - 1] + far_row[c - 1]) + 8) >> 4;
	return c == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + (3 * near_row[c + 1] + far_row[c + 1]) + 7) >> 4;
}

static long run(const uint8_t* f, long size, uint8_t* rgb, long cap, int* h, int* w, long S, uint32_t* trace, long trace_cap, int tracing) {
	frame_t F;
	memset(&g_stats, 0, sizeof g_stats);
	int r = parse(f, size, &F);
	if (r) return r;
	*h = F.h; *w = F.w;
	if (rgb && cap < 3L * F.h * F.w) return -2;
	const int mcuw = (F.w + 8 * F.hs - 1) / (8 * F.hs), mcuh = (F.h + 8 * F.vs - 1) / (8 * F.vs);
	const long nmcu = (long)mcuw * mcuh;
	const int ny = F.ncomp == 1 ? 1 : F.hs * F.vs, bpm = F.ncomp == 1 ? 1 : ny + 2;
	const long ri = F.ri > 0 && F.ri < nmcu ? F.ri : nmcu, want_int = (nmcu + ri - 1) / ri;
	uint8_t* data = (uint8_t*)calloc((size_t)size + 8, 1);
	long* iv = (long*)calloc((size_t)want_int + 2, sizeof(long));
	uint8_t* plane[3] = {0, 0, 0};
	int pw[3] = {0, 0, 0};
	for (int c = 0; c < F.ncomp; ++c) {
		pw[c] = mcuw * 8 * (c ? 1 : F.hs);
		plane[c] = (uint8_t*)calloc((size_t)pw[c] * mcuh * 8 * (c ? 1 : F.vs), 1);
	}
	long nint = 0, ret = 0;
	trace_t T = {trace, trace_cap, 0, S, 0, 0, 0, tracing};
	if (unstuff(f, size, F.scan, data, iv, want_int + 1, &nint) < 0 || nint != want_int) { ret = -1; goto done; }
	g_stats.intervals = (int32_t)nint;
	for (long j = 0; j < nint && !ret; ++j) {
		bits_t b = {data, 8 * iv[j], 8 * iv[j + 1]};
		int pred[3] = {0, 0, 0};
		const long m1 = (j + 1) * ri < nmcu ? (j + 1) * ri : nmcu;
		T.iv_end = b.end; T.sub_end = b.pos + S < b.end ? b.pos + S : b.end; T.done = 0;
		for (long m = j * ri; m < m1 && !ret; ++m) {
			for (int k = 0; k < bpm && !ret; ++k) {
				const int c = k < ny ? 0 : k - ny + 1;
				int16_t coef[64];
				int ws[64];
				memset(coef, 0, sizeof coef);
				if (decode_block(&b, &F.dc[F.td[c]], &F.ac[F.ta[c]], &pred[c], coef, &T, k)) { ret = -1; break; }
				++g_stats.blocks; ++T.done;
				trace_boundary(&T, b.pos, k + 1 == bpm ? 0 : k + 1, 0);
				for (int i = 0; i < 64; ++i) ws[ZZ[i]] = coef[ZZ[i]] * F.q[F.tq[c]][i];      /* the table is in zigzag order */
				for (int i = 0; i < 8; ++i) idct_pass(ws + i, 8, 0);
				for (int i = 0; i < 8; ++i) idct_pass(ws + 8 * i, 1, 1);
				const int hsc = c ? 1 : F.hs, vsc = c ? 1 : F.vs, sub = c ? 0 : k;
				const long bx = (m % mcuw) * hsc + sub % hsc, by = (m / mcuw) * vsc + sub / hsc;
				for (int i = 0; i < 64; ++i) plane[c][(by * 8 + i / 8) * pw[c] + bx * 8 + i % 8] = (uint8_t)clamp255(ws[i] + 128);
			}
		}
		if (!ret) {      /* how the interval ends: its pad bits and its last byte */
			int zero = 0;
			if (b.pos == b.end) { ++g_stats.unpadded; g_stats.unpadded_last = j + 1 == nint; }
			for (long p = b.pos; p < b.end; ++p) if (!((data[p >> 3] >> (7 - (p & 7))) & 1)) zero = 1;
			g_stats.pad_zero += zero;
			if (iv[j + 1] > iv[j] && data[iv[j + 1] - 1] == 0xFF) ++g_stats.end_ff;
		}
		/* what is left of the interval pads it to a byte: the last subsequence ends here */
		if (!ret && tracing) { if (T.sub_end <= T.iv_end) { T.sub_end = T.iv_end; trace_boundary(&T, b.end, 0, 0); } }
	}
	if (!ret && rgb) {
		const int cw = (F.w + F.hs - 1) / F.hs, ch = (F.h + F.vs - 1) / F.vs;
		for (int y = 0; y < F.h; ++y)
			for (int x = 0; x < F.w; ++x) {
				uint8_t* o = rgb + 3 * ((long)y * F.w + x);
				const int Y = plane[0][(long)y * pw[0] + x];
				if (F.ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; continue; }
				const int Cb = chroma(plane[1], pw[1], cw, ch, F.hs, F.vs, y, x) - 128, Cr = chroma(plane[2], pw[2], cw, ch, F.hs, F.vs, y, x) - 128;
				o[0] = (uint8_t)clamp255(Y + ((91881 * Cr + 32768) >> 16));
				o[1] = (uint8_t)clamp255(Y + ((-22554 * Cb - 46802 * Cr + 32768) >> 16));
				o[2] = (uint8_t)clamp255(Y + ((116130 * Cb + 32768) >> 16));
			}
	}
	if (!ret && tracing) ret = T.n;
done:
	free(data); free(iv);
	for (int c = 0; c < 3; ++c) free(plane[c]);
	return ret;
}

/* rgb: h x w x 3 bytes (cap of them available).  0, -1 (broken), -2 (cap too small), -4 (outside the format) */
long jpeg_dec_ref_decode(const uint8_t* f, long size, uint8_t* rgb, long cap, int* h, int* w) {
	return run(f, size, rgb, cap, h, w, 1L << 40, 0, 0, 0);
}

/* -> the number of subsequences of S bits over all intervals (their states in out, as far as cap reaches), or an error as above */
long jpeg_dec_ref_trace(const uint8_t* f, long size, long S, uint32_t* out, long cap) {
	int h, w;
	return run(f, size, 0, 0, &h, &w, S, out, cap, 1);
}
