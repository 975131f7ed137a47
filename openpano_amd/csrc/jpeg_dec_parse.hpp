// jpeg_dec_parse.hpp -- the host's header parser of the JPEG decoder: SOI .. SOS, segment by
// segment, then a search for the marker that ends the scan.  It decodes nothing: inside the entropy-coded data it only
// looks for FF xx pairs, to find EOI and to refuse a second scan or DNL.  Host C++ only; jpeg_dec.hip, the host model and
// the sanitizer program (tests/harness/jpeg_dec_fuzz.cc) include this text.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include "jpeg_dec_core.hpp"

enum { JD_OK = 0, JD_INVALID = -1, JD_UNSUPPORTED = -4 };      // OP_OK, OP_ERR_INVALID, OP_ERR_UNSUPPORTED
enum { JD_S444 = 0, JD_S420 = 1, JD_S422 = 2, JD_GREY = 3 };   // OP_JPEG_444, OP_JPEG_420, OP_JPEG_422, OP_JPEG_GREY

struct JdHeader {
	int h = 0, w = 0, ncomp = 0, sampling = -1, hs = 1, vs = 1, ri = 0;
	int tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
	bool have_q[4] = {false, false, false, false}, have_h[8] = {false, false, false, false, false, false, false, false};
	uint8_t q[4][64];          // natural order
	JdHuff huff[8];            // DC 0-3, AC 0-3
	int64_t scan_begin = 0, scan_end = 0;      // the entropy-coded data: [scan_begin, scan_end), EOI at scan_end
	std::string why;
};

inline int jd_fail(JdHeader& H, int code, const char* why) { H.why = why; return code; }

inline int jd_parse(const unsigned char* f, int64_t size, JdHeader& H) {
	static const uint8_t zz_nat[64] = JD_ZZ_NAT;
	if (!f || size < 4 || f[0] != 0xFF || f[1] != 0xD8) return jd_fail(H, JD_INVALID, "no SOI: not a JPEG file");
	int64_t pos = 2;
	bool sof = false, sos = false, jfif = false;
	int adobe_transform = -1;
	uint8_t comp_id[3] = {0, 0, 0};
	while (!sos) {
		if (pos + 2 > size) return jd_fail(H, JD_INVALID, "the file ends inside its header (no SOS)");
		if (f[pos] != 0xFF) return jd_fail(H, JD_INVALID, "no marker where a segment should begin");
		const int m = f[pos + 1];
		if (m == 0xFF) { ++pos; continue; }                          // fill byte
		if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }      // stand-alone markers
		if (m == 0xD9) return jd_fail(H, JD_INVALID, "EOI before any scan (missing SOS)");
		if (m == 0xD8 || m == 0x00) return jd_fail(H, JD_INVALID, "a stray marker in the header");
		if (pos + 4 > size) return jd_fail(H, JD_INVALID, "the file ends inside a segment header");
		const int64_t L = (int64_t)f[pos + 2] << 8 | f[pos + 3];
		if (L < 2 || pos + 2 + L > size) return jd_fail(H, JD_INVALID, "a segment runs past the end of the file");
		const unsigned char* p = f + pos + 4;
		const int64_t n = L - 2;
		if (m == 0xC0) {
			if (sof) return jd_fail(H, JD_INVALID, "two frame headers");
			if (n < 6) return jd_fail(H, JD_INVALID, "SOF0 too short");
			if (p[0] != 8) return jd_fail(H, JD_UNSUPPORTED, "sample precision is not 8 bits");
			H.h = p[1] << 8 | p[2]; H.w = p[3] << 8 | p[4]; H.ncomp = p[5];
			if (H.ncomp != 1 && H.ncomp != 3) return jd_fail(H, JD_UNSUPPORTED, "neither one nor three components");
			if (n != 6 + 3 * H.ncomp) return jd_fail(H, JD_INVALID, "SOF0 length does not match its component count");
			if (H.h == 0) return jd_fail(H, JD_UNSUPPORTED, "height 0: the frame relies on DNL");
			int samp[3] = {0x11, 0x11, 0x11};
			for (int c = 0; c < H.ncomp; ++c) {
				comp_id[c] = p[6 + 3 * c]; samp[c] = p[7 + 3 * c]; H.tq[c] = p[8 + 3 * c];
				if (H.tq[c] > 3) return jd_fail(H, JD_INVALID, "quantisation table id out of range");
			}
			if (H.ncomp == 1) {
				if (samp[0] != 0x11) return jd_fail(H, JD_UNSUPPORTED, "grey with sampling factors other than 1 x 1");
				H.sampling = JD_GREY;
			} else {
				if (samp[1] != 0x11 || samp[2] != 0x11) return jd_fail(H, JD_UNSUPPORTED, "chroma sampling other than 1 x 1");
				if (samp[0] == 0x11) H.sampling = JD_S444;
				else if (samp[0] == 0x21) { H.sampling = JD_S422; H.hs = 2; }
				else if (samp[0] == 0x22) { H.sampling = JD_S420; H.hs = 2; H.vs = 2; }
				else return jd_fail(H, JD_UNSUPPORTED, "sampling other than 4:4:4, 4:2:2 or 4:2:0");
			}
			sof = true;
		} else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xCC) ) {
			return jd_fail(H, JD_UNSUPPORTED, m == 0xC2 ? "progressive JPEG (SOF2)" : m == 0xC1 ? "extended sequential JPEG (SOF1)" :
					m >= 0xC9 ? "arithmetic-coded JPEG" : "a frame type other than baseline (SOF0)");
		} else if (m == 0xCC) {
			return jd_fail(H, JD_UNSUPPORTED, "arithmetic conditioning (DAC)");
		} else if (m == 0xC4) {
			int64_t o = 0;
			while (o < n) {
				if (o + 17 > n) return jd_fail(H, JD_INVALID, "DHT runs past its segment");
				const int tc = p[o] >> 4, th = p[o] & 15;
				if (tc > 1 || th > 3) return jd_fail(H, JD_INVALID, "Huffman table id out of range");
				int cnt = 0;
				for (int k = 0; k < 16; ++k) cnt += p[o + 1 + k];
				if (cnt > 256 || o + 17 + cnt > n) return jd_fail(H, JD_INVALID, "DHT runs past its segment");
				if (!jd_huff_build(p + o + 1, p + o + 17, cnt, H.huff[tc * 4 + th])) return jd_fail(H, JD_INVALID, "DHT counts are no prefix code");
				H.have_h[tc * 4 + th] = true;
				o += 17 + cnt;
			}
		} else if (m == 0xDB) {
			int64_t o = 0;
			while (o < n) {
				const int pq = p[o] >> 4, tq = p[o] & 15;
				if (pq == 1) return jd_fail(H, JD_UNSUPPORTED, "16-bit quantisation table");
				if (pq > 1 || tq > 3) return jd_fail(H, JD_INVALID, "quantisation table id out of range");
				if (o + 65 > n) return jd_fail(H, JD_INVALID, "DQT runs past its segment");
				for (int k = 0; k < 64; ++k) H.q[tq][zz_nat[k]] = p[o + 1 + k];
				H.have_q[tq] = true;
				o += 65;
			}
		} else if (m == 0xDD) {
			if (n != 2) return jd_fail(H, JD_INVALID, "DRI of the wrong length");
			H.ri = p[0] << 8 | p[1];
		} else if (m == 0xDC) {
			return jd_fail(H, JD_UNSUPPORTED, "DNL");
		} else if (m == 0xE0) {
			if (n >= 5 && !memcmp(p, "JFIF", 5)) jfif = true;
		} else if (m == 0xEE) {
			if (n >= 12 && !memcmp(p, "Adobe", 5)) adobe_transform = p[11];
		} else if (m == 0xDA) {
			if (!sof) return jd_fail(H, JD_INVALID, "SOS before any frame header (missing SOF)");
			if (n < 1 || n != 4 + 2 * p[0]) return jd_fail(H, JD_INVALID, "SOS of the wrong length");
			if (p[0] != H.ncomp) return jd_fail(H, JD_UNSUPPORTED, "a scan that does not interleave every component (more than one SOS)");
			for (int c = 0; c < H.ncomp; ++c) {
				if (p[1 + 2 * c] != comp_id[c]) return jd_fail(H, JD_UNSUPPORTED, "scan components not in the frame's order");
				H.td[c] = p[2 + 2 * c] >> 4; H.ta[c] = p[2 + 2 * c] & 15;
				if (H.td[c] > 3 || H.ta[c] > 3) return jd_fail(H, JD_INVALID, "Huffman table id out of range");
			}
			const unsigned char* e = p + 1 + 2 * H.ncomp;
			if (e[0] != 0 || e[1] != 63 || e[2] != 0) return jd_fail(H, JD_UNSUPPORTED, "spectral selection or successive approximation");
			sos = true;
		}
		// everything else (APPn, COM, JPGn, reserved) is skipped by its length
		pos += 2 + L;
	}
	if (adobe_transform == 0 && H.ncomp == 3) return jd_fail(H, JD_UNSUPPORTED, "Adobe APP14 with transform 0 (RGB components)");
	if (!jfif && adobe_transform < 0 && H.ncomp == 3 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
		return jd_fail(H, JD_UNSUPPORTED, "components named R, G, B without JFIF (RGB components)");
	for (int c = 0; c < H.ncomp; ++c) {
		if (!H.have_q[H.tq[c]]) return jd_fail(H, JD_INVALID, "missing DQT: a component names a table the file does not define");
		if (!H.have_h[H.td[c]] || !H.have_h[4 + H.ta[c]]) return jd_fail(H, JD_INVALID, "missing DHT: the scan names a table the file does not define");
	}
	H.scan_begin = pos;
	// the marker that ends the scan: stuffed bytes and RSTn pass, EOI ends it, SOS / DNL are refused, any other marker
	// is left to the device, which flags it
	int64_t i = pos;
	for (;;) {
		const void* hit = i < size ? memchr(f + i, 0xFF, (size_t)(size - i)) : nullptr;
		if (!hit || (const unsigned char*)hit - f + 1 >= size) return jd_fail(H, JD_INVALID, "missing EOI");
		i = (const unsigned char*)hit - f;
		const int m = f[i + 1];
		if (m == 0xD9) break;
		if (m == 0xDA) return jd_fail(H, JD_UNSUPPORTED, "more than one SOS");
		if (m == 0xDC) return jd_fail(H, JD_UNSUPPORTED, "DNL");
		i += m == 0xFF ? 1 : 2;
	}
	H.scan_end = i;
	if (H.scan_end - H.scan_begin >= ((int64_t)1 << 29)) return jd_fail(H, JD_UNSUPPORTED, "a scan of 512 MiB or more");
	if (H.h < 2 || H.w < 2) return jd_fail(H, JD_INVALID, "h or w below 2");
	return JD_OK;
}

// the device's description of a parsed file, but for the offsets into the batch's buffers
inline void jd_describe(const JdHeader& H, JdImage& I) {
	memset(&I, 0, sizeof I);
	I.h = H.h; I.w = H.w; I.hs = H.hs; I.vs = H.vs; I.ncomp = H.ncomp;
	I.mcuw = (H.w + 8 * H.hs - 1) / (8 * H.hs); I.mcuh = (H.h + 8 * H.vs - 1) / (8 * H.vs);
	I.nmcu = (uint32_t)I.mcuw * (uint32_t)I.mcuh;
	I.bpm = H.ncomp == 1 ? 1u : (uint32_t)(H.hs * H.vs + 2);
	I.nblocks = I.nmcu * I.bpm;
	I.ri = H.ri > 0 && (uint32_t)H.ri < I.nmcu ? (uint32_t)H.ri : I.nmcu;
	I.nint = (I.nmcu + I.ri - 1) / I.ri;
	I.in_len = (uint32_t)(H.scan_end - H.scan_begin);
	for (int c = 0; c < H.ncomp; ++c) {
		I.plane_w[c] = I.mcuw * 8 * (c ? 1 : H.hs); I.plane_h[c] = I.mcuh * 8 * (c ? 1 : H.vs);
		memcpy(I.q[c], H.q[H.tq[c]], 64);
	}
	const int ny = H.ncomp == 1 ? 1 : H.hs * H.vs;
	for (int k = 0; k < (int)I.bpm; ++k) {
		const int c = k < ny ? 0 : k - ny + 1;
		I.kinfo[k] = (uint8_t)(c | H.td[c] << 2 | H.ta[c] << 4);
	}
	for (int t = 0; t < 8; ++t) {
		if (H.have_h[t]) I.huff[t] = H.huff[t];
		else for (int l = 0; l <= 16; ++l) I.huff[t].lim[l] = 0;      // never selected; every code is invalid
	}
}
