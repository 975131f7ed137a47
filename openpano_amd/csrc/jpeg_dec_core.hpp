// jpeg_dec_core.hpp -- the per-symbol step, the state and the pass-B convergence rule of the self-synchronising baseline
// JPEG Huffman decode.  One text for the kernels of jpeg_dec.hip, for the host model that
// tests/test_jpeg_dec_cpu.py runs (tests/harness/jpeg_dec_fuzz.cc) and for the sanitizer program built from the same file.
// Plain C++ with no dependency but <stdint.h> and the macros of jpeg_tables.hpp.
#pragma once
#include <stdint.h>
#include "jpeg_tables.hpp"

#if defined(__HIPCC__)
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

#define JD_S_DEFAULT 1024      // bits of a subsequence
#define JD_S_MAX 65536         // a subsequence completes at most S / 2 + 1 blocks, which must fit the state's 16-bit count
#define JD_PAD 8               // bytes past the compacted data that a window read may touch

// bits of an image's error word
enum { JD_ERR_MARKER = 1,      // a marker other than RSTn in the entropy-coded data, or RSTn out of order
       JD_ERR_INTERVALS = 2,   // the number of restart intervals is not the frame's
       JD_ERR_CODE = 4,        // no Huffman code matches (true path)
       JD_ERR_INDEX = 8,       // a run leads past coefficient 63 (true path)
       JD_ERR_CAT = 16,        // DC category above 11 or AC category above 10 (true path)
       JD_ERR_END = 32,        // a symbol runs past its restart interval (true path)
       JD_ERR_COUNT = 64,      // an interval does not hold the frame's number of blocks
       JD_ERR_CAP = 128 };     // more subsequences than the host sized for (cannot happen: a consistency check)
// result bits of jd_step that are no errors
enum { JD_BLOCK_DONE = 1 << 8, JD_COEF = 1 << 9, JD_ZRL = 1 << 10, JD_EOB = 1 << 11 };

#define JD_ZZ_NAT JPEG_ZZ_NAT      // zigzag position -> natural index: the encoder's table (jpeg_tables.hpp)

// One Huffman table as a length-indexed lookup.  The canonical codes of length L, left-justified in 16 bits, fill
// [lim[L - 1], lim[L]); off[L] + (the L-bit code) is the symbol's place in vals.
struct JdHuff { uint32_t lim[17]; int32_t off[17]; uint8_t vals[256]; };

// false: the counts describe more codes than a prefix code of that length can hold
inline bool jd_huff_build(const uint8_t counts[16], const uint8_t* vals, int nvals, JdHuff& t) {
	uint32_t code = 0; int k = 0;
	t.lim[0] = 0; t.off[0] = 0;
	for (int len = 1; len <= 16; ++len) {
		t.off[len] = k - (int32_t)code;
		code += counts[len - 1]; k += counts[len - 1];
		if (code > (1u << len) || k > 256) return false;
		t.lim[len] = code << (16 - len);
		code <<= 1;
	}
	for (int i = 0; i < 256; ++i) t.vals[i] = i < nvals && i < k ? vals[i] : 0;
	return true;
}

// what a block of the MCU decodes with: component (bits 0-1), DC table (2-3), AC table (4-5)
JD_HD int jd_kinfo_comp(uint8_t v) { return v & 3; }
JD_HD int jd_kinfo_dc(uint8_t v) { return (v >> 2) & 3; }
JD_HD int jd_kinfo_ac(uint8_t v) { return 4 + ((v >> 4) & 3); }

// The decoder's state between two symbols: bit position in the image's compacted data, block in the MCU, zigzag position
// (0: a DC symbol is next), and the blocks completed since the subsequence was entered.
struct JdCur { uint32_t pos; int k, zz; uint32_t n; };
// packed for the exit-state arrays: pos 63..32, n 31..16, k 11..8, zz 6..1, bit 0 = "changed in the round that wrote it"
JD_HD uint64_t jd_pack(const JdCur& c, int chg) {
	return (uint64_t)c.pos << 32 | (uint64_t)(c.n & 0xFFFFu) << 16 | (uint64_t)(c.k & 15) << 8 | (uint64_t)(c.zz & 63) << 1 | (uint64_t)(chg & 1);
}
JD_HD JdCur jd_unpack(uint64_t v) { JdCur c; c.pos = (uint32_t)(v >> 32); c.n = (uint32_t)(v >> 16) & 0xFFFFu; c.k = (int)(v >> 8) & 15; c.zz = (int)(v >> 1) & 63; return c; }
JD_HD bool jd_same_exit(uint64_t a, uint64_t b) { return ((a ^ b) & 0xFFFFFFFF0000FFFEull) == 0; }      // pos, k, zz
JD_HD uint32_t jd_count(uint64_t v) { return (uint32_t)(v >> 16) & 0xFFFFu; }

// 32 bits from bit `pos`, MSB first; touches bytes pos / 8 .. pos / 8 + 4
JD_HD uint32_t jd_peek32(const uint8_t* d, uint32_t pos) {
	const uint8_t* p = d + (pos >> 3);
	const uint64_t v = (uint64_t)p[0] << 32 | (uint64_t)p[1] << 24 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 8 | (uint64_t)p[4];
	return (uint32_t)(v >> (8 - (pos & 7)));
}

// One symbol.  d: compacted data; end: the restart interval's last bit + 1; huff: 8 tables (DC 0-3, AC 0-3); kinfo: bpm entries.
// On JD_COEF, `val` belongs at zigzag position `idx` of the block in progress (the DC as a difference).  Every path
// advances: an invalid code consumes 16 bits and a run past coefficient 63 ends the block, so a speculative decode never
// stalls; a symbol that would pass `end` is not taken and the position becomes `end`.  The error bits matter on the true
// path only.
JD_HD uint32_t jd_step(const uint8_t* d, uint32_t end, const JdHuff* huff, const uint8_t* kinfo, int bpm, JdCur& c, int& idx, int& val) {
	const uint32_t w = jd_peek32(d, c.pos);
	const uint8_t ki = kinfo[c.k];
	const JdHuff& t = huff[c.zz == 0 ? jd_kinfo_dc(ki) : jd_kinfo_ac(ki)];
	const uint32_t w16 = w >> 16;
	int len = 1;
	while (len <= 16 && w16 >= t.lim[len]) ++len;
	if (len > 16) {
		c.pos = end - c.pos < 16 ? end : c.pos + 16;
		return JD_ERR_CODE;
	}
	const int sym = t.vals[(t.off[len] + (int32_t)(w16 >> (16 - len))) & 255];
	const int s = sym & 15, r = sym >> 4;
	if (end - c.pos < (uint32_t)(len + s)) { c.pos = end; return JD_ERR_END; }
	c.pos += (uint32_t)(len + s);
	uint32_t fl = 0;
	int v = 0;
	if (s) {
		v = (int)((w << len) >> (32 - s));
		if (v < (1 << (s - 1))) v = v - (1 << s) + 1;      // EXTEND
	}
	int zz = c.zz;
	if (zz == 0) {
		if (s > 11) fl |= JD_ERR_CAT;
		idx = 0; val = v; fl |= JD_COEF; zz = 1;
	} else if (s == 0) {
		if (r == 15) { if (zz + 16 > 63) fl |= JD_ERR_INDEX; zz += 16; fl |= JD_ZRL; }
		else { zz = 64; fl |= JD_EOB; }
	} else {
		if (s > 10) fl |= JD_ERR_CAT;
		zz += r;
		if (zz > 63) fl |= JD_ERR_INDEX;
		else { idx = zz; val = v; fl |= JD_COEF; }
		++zz;
	}
	if (zz >= 64) { zz = 0; c.k = c.k + 1 == bpm ? 0 : c.k + 1; ++c.n; fl |= JD_BLOCK_DONE; }
	c.zz = zz;
	return fl;
}

// decode from c to the first symbol boundary at or past sub_end (a subsequence's last bit + 1, never past `end`)
JD_HD void jd_run(const uint8_t* d, uint32_t sub_end, uint32_t end, const JdHuff* huff, const uint8_t* kinfo, int bpm, JdCur& c) {
	while (c.pos < sub_end) { int idx, val; (void)jd_step(d, end, huff, kinfo, bpm, c, idx, val); }
}

// Behind an interval's last block (pass C, on the true path) only the bits that pad the interval to a byte may follow: fewer
// than eight, in the interval's last subsequence, at a block boundary.  A whole byte or more there is a block too many, whatever S is.
JD_HD bool jd_tail_is_padding(bool last_sub, const JdCur& c, uint32_t end) { return last_sub && c.zz == 0 && end - c.pos < 8; }

// One subsequence in one round of the synchronisation.  Round 0 (pass A) decodes from the subsequence's first bit in state
// (block 0, position 0), which is the true state for an interval's first subsequence.  A later round (pass B) re-decodes
// from the predecessor's exit state if that changed in the round before, and marks its own exit as changed when its
// position, block or zigzag position differ from what it stored; otherwise it keeps what it has.  `pred` and `own` are what
// the round before stored.  After round r the subsequences 0..r of every interval hold their true exit state, so an
// interval of L subsequences needs no round past L - 1, and the rounds end when one changes nothing.
JD_HD uint64_t jd_sub_round(const uint8_t* d, uint32_t sub_begin, uint32_t sub_end, uint32_t end, bool first_of_interval, int round,
		uint64_t pred, uint64_t own, const JdHuff* huff, const uint8_t* kinfo, int bpm) {
	JdCur c;
	if (round == 0) {
		c.pos = sub_begin; c.k = 0; c.zz = 0; c.n = 0;
		jd_run(d, sub_end, end, huff, kinfo, bpm, c);
		return jd_pack(c, 1);
	}
	if (first_of_interval || !(pred & 1)) return own & ~1ull;
	c = jd_unpack(pred); c.n = 0;
	jd_run(d, sub_end, end, huff, kinfo, bpm, c);
	const uint64_t r = jd_pack(c, 0);
	return r | (jd_same_exit(r, own) ? 0ull : 1ull);
}

// subsequences of an interval of `bits` bits
JD_HD uint32_t jd_nsub(uint32_t bits, uint32_t S) { const uint32_t n = bits / S + (bits % S ? 1u : 0u); return n ? n : 1u; }

// ---- IDCT, upsampling, colour: the integer rules of libjpeg's default decode ----
JD_HD int jd_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// one pass of jpeg_idct_islow over eight values; SHIFT = 11 (columns, into the workspace) or 18 (rows)
template <int SHIFT>
JD_HD void jd_idct_pass(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, int (&o)[8]) {
	const int z1 = (i2 + i6) * 4433;
	const int e2 = z1 - i6 * 15137, e3 = z1 + i2 * 6270;
	const int e0 = (int)((unsigned)(i0 + i4) << 13), e1 = (int)((unsigned)(i0 - i4) << 13);
	const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
	int t0 = i7, t1 = i5, t2 = i3, t3 = i1;
	int y1 = t0 + t3, y2 = t1 + t2, y3 = t0 + t2, y4 = t1 + t3;
	const int y5 = (y3 + y4) * 9633;
	t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
	y1 *= -7373; y2 *= -20995; y3 *= -16069; y4 *= -3196;
	y3 += y5; y4 += y5;
	t0 += y1 + y3; t1 += y2 + y4; t2 += y2 + y3; t3 += y1 + y4;
	const int rnd = 1 << (SHIFT - 1);
	o[0] = (t10 + t3 + rnd) >> SHIFT; o[7] = (t10 - t3 + rnd) >> SHIFT;
	o[1] = (t11 + t2 + rnd) >> SHIFT; o[6] = (t11 - t2 + rnd) >> SHIFT;
	o[2] = (t12 + t1 + rnd) >> SHIFT; o[5] = (t12 - t1 + rnd) >> SHIFT;
	o[3] = (t13 + t0 + rnd) >> SHIFT; o[4] = (t13 - t0 + rnd) >> SHIFT;
}

// chroma sample for output pixel (y, x) from a plane of cw x ch real samples with row pitch `pitch`; hs, vs in {1, 2}.
// libjpeg takes the fancy (triangle) filters only where the downsampled width exceeds 2, and replicates otherwise.
JD_HD int jd_chroma(const uint8_t* p, int pitch, int cw, int ch, int hs, int vs, int y, int x) {
	if (hs == 1) return p[(long long)y * pitch + x];
	const int c = x >> 1;
	if (vs == 1) {
		const uint8_t* in = p + (long long)y * pitch;
		if (cw <= 2) return in[c];
		if (!(x & 1)) return c == 0 ? in[0] : (3 * in[c] + in[c - 1] + 1) >> 2;
		return c == cw - 1 ? in[c] : (3 * in[c] + in[c + 1] + 2) >> 2;
	}
	const int r = y >> 1;
	if (cw <= 2) return p[(long long)r * pitch + c];
	int far = (y & 1) ? r + 1 : r - 1;
	far = far < 0 ? 0 : far > ch - 1 ? ch - 1 : far;
	const uint8_t* n = p + (long long)r * pitch; const uint8_t* f = p + (long long)far * pitch;
	const int cur = 3 * n[c] + f[c];
	if (!(x & 1)) return c == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * n[c - 1] + f[c - 1] + 8) >> 4;
	return c == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * n[c + 1] + f[c + 1] + 7) >> 4;
}

JD_HD void jd_ycc_rgb(int Y, int Cb, int Cr, uint8_t* o) {
	Cb -= 128; Cr -= 128;
	o[0] = (uint8_t)jd_clamp255(Y + ((91881 * Cr + 32768) >> 16));
	o[1] = (uint8_t)jd_clamp255(Y + ((-22554 * Cb - 46802 * Cr + 32768) >> 16));
	o[2] = (uint8_t)jd_clamp255(Y + ((116130 * Cb + 32768) >> 16));
}

// ---- what the host tells the device about one file ----
struct JdImage {
	uint64_t in_off, cmp_off, coef_off, out_off, plane_off[3];      // bytes into the batch's buffers (coef_off in int16 units)
	uint32_t in_len, iv_off, sub_off, sub_cap;
	uint32_t nint, ri, nmcu, nblocks, bpm;      // ri: MCUs of a restart interval (nmcu when the file has none)
	int32_t h, w, mcuw, mcuh, hs, vs, ncomp;
	int32_t plane_w[3], plane_h[3];
	uint8_t kinfo[8];
	uint8_t q[3][64];                           // per component, natural order
	JdHuff huff[8];
};
struct JdStatus { uint32_t err, ncompact, nsub, maxl, rounds, pad0, pad1, pad2; };
