/* jpeg_ref.c -- the serial restatement of openpano_amd/csrc/jpeg.hip: baseline JPEG, 4:4:4 or 4:2:0,
 * Annex K Huffman tables, one restart interval per OP_JPEG_RI_444 / OP_JPEG_RI_420 MCUs.  Integer arithmetic only, written as
 * plain loops over MCUs, blocks and coefficients; its files are compared byte for byte with libjpeg's (tests/test_jpeg_ref_cpu.py)
 * and with the device's (tests/test_gpu_jpeg.py).  jpeg_ref_stats says what the last encode went through. */
#include <assert.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef OP_JPEG_RI_444
#define OP_JPEG_RI_444 32
#endif
#ifndef OP_JPEG_RI_420
#define OP_JPEG_RI_420 8
#endif
#define BLOCK_BYTES 208      /* worst case of one block: 20 + 63 * 26 bits */

typedef struct {
	int32_t stuffed, stuffed_pad, zrl, no_eob, dummy_right, dummy_bottom, max_dc_cat, max_ac_cat, intervals, max_interval_bytes;
} jpeg_ref_stats_t;
static jpeg_ref_stats_t g_stats;
void jpeg_ref_stats(jpeg_ref_stats_t* s) { *s = g_stats; }

static const uint8_t K1[64] = {
	16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
	18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t K2[64] = {
	17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
	99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
/* zigzag position -> natural index */
static const uint8_t ZZ[64] = {
	0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
	35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t DC_COUNTS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t AC_COUNTS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t AC_VALS[2][162] = {{
	1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114,
	130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89,
	90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149,
	150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198,
	199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245,
	246, 247, 248, 249, 250}, {
	0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209,
	10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
	89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147,
	148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196,
	197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245,
	246, 247, 248, 249, 250}};

typedef struct { uint16_t code[256]; uint8_t size[256]; } huff_t;

static void huff_make(const uint8_t* counts, const uint8_t* vals, huff_t* t) {
	memset(t, 0, sizeof *t);
	unsigned code = 0; int k = 0;
	for (int len = 1; len <= 16; ++len) {
		for (int i = 0; i < counts[len - 1]; ++i) { t->code[vals[k]] = (uint16_t)code++; t->size[vals[k]] = (uint8_t)len; ++k; }
		code <<= 1;
	}
}

int jpeg_ref_interval(int subsampling) { return subsampling == 0 ? OP_JPEG_RI_444 : subsampling == 1 ? OP_JPEG_RI_420 : -1; }
/* bytes in which an interval is assembled: every block at its worst case, every byte stuffed */
int jpeg_ref_slot(int subsampling) { return 2 * BLOCK_BYTES * jpeg_ref_interval(subsampling) * (subsampling == 0 ? 3 : 6); }

static void quant_tables(int quality, uint16_t q[2][64]) {
	const int S = quality < 50 ? 5000 / quality : 200 - 2 * quality;
	for (int k = 0; k < 64; ++k) {
		int a = (K1[k] * S + 50) / 100, b = (K2[k] * S + 50) / 100;
		q[0][k] = (uint16_t)(a < 1 ? 1 : a > 255 ? 255 : a);
		q[1][k] = (uint16_t)(b < 1 ? 1 : b > 255 ? 255 : b);
	}
}

static int put16(uint8_t* o, int v) { o[0] = (uint8_t)(v >> 8); o[1] = (uint8_t)v; return 2; }

/* SOI .. SOS; at most 640 bytes */
static long write_header(uint8_t* o, int h, int w, int subsampling, const uint16_t q[2][64]) {
	long n = 0;
	static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
	memcpy(o, app0, sizeof app0); n += sizeof app0;
	for (int t = 0; t < 2; ++t) {
		o[n++] = 0xFF; o[n++] = 0xDB; n += put16(o + n, 67); o[n++] = (uint8_t)t;
		for (int k = 0; k < 64; ++k) o[n++] = (uint8_t)q[t][ZZ[k]];
	}
	o[n++] = 0xFF; o[n++] = 0xC0; n += put16(o + n, 17); o[n++] = 8; n += put16(o + n, h); n += put16(o + n, w); o[n++] = 3;
	for (int c = 0; c < 3; ++c) { o[n++] = (uint8_t)(c + 1); o[n++] = (c == 0 && subsampling == 1) ? 0x22 : 0x11; o[n++] = c ? 1 : 0; }
	for (int t = 0; t < 4; ++t) {      /* DC0, AC0, DC1, AC1 */
		const int cls = t & 1, id = t >> 1, nv = cls ? 162 : 12;
		o[n++] = 0xFF; o[n++] = 0xC4; n += put16(o + n, 2 + 1 + 16 + nv); o[n++] = (uint8_t)(cls << 4 | id);
		memcpy(o + n, cls ? AC_COUNTS[id] : DC_COUNTS[id], 16); n += 16;
		memcpy(o + n, cls ? AC_VALS[id] : DC_VALS, (size_t)nv); n += nv;
	}
	o[n++] = 0xFF; o[n++] = 0xDD; n += put16(o + n, 4); n += put16(o + n, jpeg_ref_interval(subsampling));
	static const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
	memcpy(o + n, sos, sizeof sos); n += sizeof sos;
	return n;
}

long jpeg_ref_bound(int h, int w, int subsampling) {
	const int m = subsampling == 0 ? 8 : 16, ri = jpeg_ref_interval(subsampling);
	if (ri < 0) return -1;
	const long nmcu = (long)((h + m - 1) / m) * ((w + m - 1) / m), nint = (nmcu + ri - 1) / ri;
	return 640 + nint * (jpeg_ref_slot(subsampling) + 2) + 2;
}

static int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

/* one pass of the IJG slow-integer transform over d[0], d[stride], ..; pass 0 = rows, 1 = columns */
static void fdct_pass(int* d, int stride, int pass) {
	const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride], d7 = d[7 * stride];
	const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
	const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
	const int s = pass ? 15 : 11;
	d[0] = pass ? descale(t10 + t11, 2) : (t10 + t11) * 4;
	d[4 * stride] = pass ? descale(t10 - t11, 2) : (t10 - t11) * 4;
	const int z = (t12 + t13) * 4433;
	d[2 * stride] = descale(z + t13 * 6270, s);
	d[6 * stride] = descale(z - t12 * 15137, s);
	const int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
	const int y3 = z5 - z3 * 16069, y4 = z5 - z4 * 3196;
	d[7 * stride] = descale(t4 * 2446 - z1 * 7373 + y3, s);
	d[5 * stride] = descale(t5 * 16819 - z2 * 20995 + y4, s);
	d[3 * stride] = descale(t6 * 25172 - z2 * 20995 + y3, s);
	d[stride] = descale(t7 * 12299 - z1 * 7373 + y4, s);
}

/* samples (0..255, natural order) -> quantised coefficients in zigzag order */
static void transform(const int* samples, const uint16_t* q, int16_t* zz) {
	int d[64];
	for (int k = 0; k < 64; ++k) d[k] = samples[k] - 128;
	for (int r = 0; r < 8; ++r) fdct_pass(d + 8 * r, 1, 0);
	for (int c = 0; c < 8; ++c) fdct_pass(d + c, 8, 1);
	for (int k = 0; k < 64; ++k) {
		const int c = d[ZZ[k]], qv = 8 * q[ZZ[k]];
		const int a = ((c < 0 ? -c : c) + (qv >> 1)) / qv;
		zz[k] = (int16_t)(c < 0 ? -a : a);
	}
}

typedef struct { uint8_t* p; long bits; } bitw_t;      /* MSB first into zeroed bytes */
static void put_bits(bitw_t* b, unsigned v, int n) {
	for (int i = n - 1; i >= 0; --i, ++b->bits)
		if ((v >> i) & 1) b->p[b->bits >> 3] |= (uint8_t)(0x80 >> (b->bits & 7));
}
static int bit_length(int v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }

static void encode_block(bitw_t* b, const int16_t* zz, int* pred, const huff_t* dc, const huff_t* ac) {
	const int d = zz[0] - *pred;
	*pred = zz[0];
	int cat = bit_length(d < 0 ? -d : d);
	assert(cat <= 11);
	if (cat > g_stats.max_dc_cat) g_stats.max_dc_cat = cat;
	put_bits(b, dc->code[cat], dc->size[cat]);
	put_bits(b, (unsigned)(d > 0 ? d : d - 1) & ((1u << cat) - 1), cat);
	int run = 0;
	for (int k = 1; k < 64; ++k) {
		const int v = zz[k];
		if (!v) { ++run; continue; }
		while (run >= 16) { put_bits(b, ac->code[0xF0], ac->size[0xF0]); run -= 16; ++g_stats.zrl; }
		cat = bit_length(v < 0 ? -v : v);
		assert(cat <= 10);
		if (cat > g_stats.max_ac_cat) g_stats.max_ac_cat = cat;
		put_bits(b, ac->code[run << 4 | cat], ac->size[run << 4 | cat]);
		put_bits(b, (unsigned)(v > 0 ? v : v - 1) & ((1u << cat) - 1), cat);
		run = 0;
	}
	if (run) put_bits(b, ac->code[0], ac->size[0]); else ++g_stats.no_eob;
}

static void ycc(const uint8_t* p, int* y, int* cb, int* cr) {
	const int R = p[0], G = p[1], B = p[2];
	*y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
	*cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
	*cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}
static const uint8_t* pixel(const uint8_t* rgb, int h, int w, int y, int x) {      /* edges repeat */
	if (y > h - 1) y = h - 1;
	if (x > w - 1) x = w - 1;
	return rgb + 3 * ((long)y * w + x);
}

long jpeg_ref_encode(const uint8_t* rgb, int h, int w, int quality, int subsampling, uint8_t* out, long cap) {
	if (h < 1 || w < 1 || h > 65535 || w > 65535 || quality < 1 || quality > 100 || (subsampling != 0 && subsampling != 1)) return -1;
	if (cap < jpeg_ref_bound(h, w, subsampling)) return -2;
	memset(&g_stats, 0, sizeof g_stats);
	uint16_t q[2][64];
	quant_tables(quality, q);
	huff_t dc[2], ac[2];
	for (int t = 0; t < 2; ++t) { huff_make(DC_COUNTS[t], DC_VALS, &dc[t]); huff_make(AC_COUNTS[t], AC_VALS[t], &ac[t]); }
	long n = write_header(out, h, w, subsampling, q);
	const int m = subsampling == 0 ? 8 : 16, ri = jpeg_ref_interval(subsampling), slot = jpeg_ref_slot(subsampling);
	const int mw = (w + m - 1) / m, mh = (h + m - 1) / m, bw8 = (w + 7) / 8, bh8 = (h + 7) / 8, ch = (h + 1) / 2;
	const long nmcu = (long)mw * mh;
	uint8_t* buf = (uint8_t*)malloc((size_t)slot / 2 + 8);
	int samples[64]; int16_t zz[64];
	for (long m0 = 0, iv = 0; m0 < nmcu; m0 += ri, ++iv) {
		const long m1 = m0 + ri < nmcu ? m0 + ri : nmcu;
		memset(buf, 0, (size_t)slot / 2 + 8);
		bitw_t b = {buf, 0};
		int pred[3] = {0, 0, 0};
		for (long mi = m0; mi < m1; ++mi) {
			const int my = (int)(mi / mw), mx = (int)(mi % mw);
			if (subsampling == 0) {
				for (int c = 0; c < 3; ++c) {
					for (int k = 0; k < 64; ++k) {
						int v[3];
						ycc(pixel(rgb, h, w, my * 8 + (k >> 3), mx * 8 + (k & 7)), &v[0], &v[1], &v[2]);
						samples[k] = v[c];
					}
					transform(samples, q[c ? 1 : 0], zz);
					encode_block(&b, zz, &pred[c], &dc[c ? 1 : 0], &ac[c ? 1 : 0]);
				}
				continue;
			}
			for (int k4 = 0; k4 < 4; ++k4) {      /* Y00 Y01 Y10 Y11 */
				const int bx = mx * 2 + (k4 & 1), by = my * 2 + (k4 >> 1);
				if (bx >= bw8 || by >= bh8) {     /* dummy: DC of the block before it (difference 0), no AC */
					if (by >= bh8) ++g_stats.dummy_bottom; else ++g_stats.dummy_right;
					put_bits(&b, dc[0].code[0], dc[0].size[0]);
					put_bits(&b, ac[0].code[0], ac[0].size[0]);
					continue;
				}
				for (int k = 0; k < 64; ++k) {
					int cb, cr;
					ycc(pixel(rgb, h, w, by * 8 + (k >> 3), bx * 8 + (k & 7)), &samples[k], &cb, &cr);
				}
				transform(samples, q[0], zz);
				encode_block(&b, zz, &pred[0], &dc[0], &ac[0]);
			}
			for (int c = 1; c < 3; ++c) {
				for (int k = 0; k < 64; ++k) {
					int cy = my * 8 + (k >> 3);
					const int cx = mx * 8 + (k & 7);
					if (cy > ch - 1) cy = ch - 1;      /* downsampled rows repeat; the full-resolution height is padded to even only */
					int sum = 0;
					for (int j = 0; j < 4; ++j) {
						int v[3];
						ycc(pixel(rgb, h, w, 2 * cy + (j >> 1), 2 * cx + (j & 1)), &v[0], &v[1], &v[2]);
						sum += v[c];
					}
					samples[k] = (sum + ((cx & 1) ? 2 : 1)) >> 2;
				}
				transform(samples, q[1], zz);
				encode_block(&b, zz, &pred[c], &dc[1], &ac[1]);
			}
		}
		const int pad = (int)(-b.bits & 7);
		put_bits(&b, (1u << pad) - 1, pad);
		const long nb = b.bits >> 3;
		long before = n;
		for (long i = 0; i < nb; ++i) {
			out[n++] = buf[i];
			if (buf[i] == 0xFF) { out[n++] = 0; ++g_stats.stuffed; if (i == nb - 1 && pad) ++g_stats.stuffed_pad; }
		}
		if (n - before > g_stats.max_interval_bytes) g_stats.max_interval_bytes = (int32_t)(n - before);
		assert(n - before <= slot);
		++g_stats.intervals;
		out[n++] = 0xFF;
		out[n++] = m1 < nmcu ? (uint8_t)(0xD0 + (iv & 7)) : 0xD9;
	}
	free(buf);
	return n;
}
