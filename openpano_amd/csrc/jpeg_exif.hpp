// jpeg_exif.hpp -- the host's EXIF reader of the JPEG decoder: the orientation (tag 0x0112) and
// FocalLengthIn35mmFilm (tag 0xA405) of a camera file.  Plain host C++, no device code; jpeg_dec.hip and the sanitizer program
// (tests/harness/jpeg_exif_fuzz.cc) include this text.  The rules:
//   segment walk   from SOI to the first SOS, segment by segment, as jd_parse does (fill bytes, stand-alone markers);
//   which segment  the first APP1 whose payload starts with 45 78 69 66 00 00 ("Exif\0\0") and holds at least 8 more bytes;
//                  later APP1s (XMP, a second Exif) are ignored, and so is every APP1 before it that is no Exif;
//   TIFF header    follows those six bytes: II 2A 00 or MM 00 2A, then the offset of IFD0.  Every offset is relative to the
//                  TIFF header and is checked against the end of this segment's payload before anything is read through it;
//   IFD layout     a 16-bit entry count, then 12-byte entries (tag, type, count, value / offset); the count is clipped to
//                  the entries that fit in the segment;
//   what is visited  two IFDs at most: IFD0 and the Exif sub-IFD that IFD0's tag 0x8769 (LONG, count 1) points to.  No
//                  next-IFD link is followed, no thumbnail IFD, no loop;
//   orientation    tag 0x0112 in IFD0, SHORT or LONG, count 1, value 1..8; anything else gives 1;
//   focal length   tag 0xA405, SHORT, count 1, looked up in the sub-IFD first and then in IFD0; absent or 0 gives 0;
//   malformed EXIF is never an error: bad magic, an offset past the segment, a count of 0, a truncated entry, a segment
//                  that runs past the file all give orientation 1 and focal 0.  Only a file without SOI is refused
//                  (JX_INVALID, as jd_parse refuses it).
#pragma once
#include <stdint.h>
#include <string.h>

enum { JX_OK = 0, JX_INVALID = -1 };      // OP_OK, OP_ERR_INVALID

struct JxExif { int orientation = 1, focal35 = 0; };

// a TIFF block of n bytes at t: every read goes through these, which check the range first
struct JxTiff {
	const unsigned char* t; int64_t n; bool le;
	bool u16(int64_t o, uint32_t& v) const {
		if (o < 0 || o + 2 > n) return false;
		v = le ? (uint32_t)t[o] | (uint32_t)t[o + 1] << 8 : (uint32_t)t[o] << 8 | (uint32_t)t[o + 1];
		return true;
	}
	bool u32(int64_t o, uint32_t& v) const {
		if (o < 0 || o + 4 > n) return false;
		v = le ? (uint32_t)t[o] | (uint32_t)t[o + 1] << 8 | (uint32_t)t[o + 2] << 16 | (uint32_t)t[o + 3] << 24
		       : (uint32_t)t[o] << 24 | (uint32_t)t[o + 1] << 16 | (uint32_t)t[o + 2] << 8 | (uint32_t)t[o + 3];
		return true;
	}
};

enum { JX_SHORT = 3, JX_LONG = 4 };

// the first entry of the IFD at `off` with this tag, count 1 and a type of the mask (bit JX_SHORT, bit JX_LONG): its value
inline bool jx_find(const JxTiff& T, int64_t off, uint32_t tag, uint32_t types, uint32_t& value) {
	uint32_t cnt;
	if (!T.u16(off, cnt)) return false;
	const int64_t fit = (T.n - off - 2) / 12;
	if ((int64_t)cnt > fit) cnt = (uint32_t)fit;
	for (uint32_t k = 0; k < cnt; ++k) {
		const int64_t e = off + 2 + 12 * (int64_t)k;
		uint32_t tg, ty, c, v;
		if (!T.u16(e, tg) || !T.u16(e + 2, ty) || !T.u32(e + 4, c)) return false;
		if (tg != tag) continue;
		if (c != 1 || ty > 31 || !(types >> ty & 1)) return false;
		if (!(ty == JX_SHORT ? T.u16(e + 8, v) : T.u32(e + 8, v))) return false;
		value = v;
		return true;
	}
	return false;
}

// p: the n bytes that follow "Exif\0\0" in the segment
inline void jx_tiff(const unsigned char* p, int64_t n, JxExif& X) {
	if (n < 8) return;
	JxTiff T{p, n, false};
	if (p[0] == 'I' && p[1] == 'I' && p[2] == 0x2A && p[3] == 0x00) T.le = true;
	else if (p[0] == 'M' && p[1] == 'M' && p[2] == 0x00 && p[3] == 0x2A) T.le = false;
	else return;
	uint32_t ifd0, v, sub;
	if (!T.u32(4, ifd0) || (int64_t)ifd0 + 2 > n) return;
	if (jx_find(T, ifd0, 0x0112, 1u << JX_SHORT | 1u << JX_LONG, v) && v >= 1 && v <= 8) X.orientation = (int)v;
	bool have = false;
	if (jx_find(T, ifd0, 0x8769, 1u << JX_LONG, sub) && (int64_t)sub + 2 <= n) have = jx_find(T, sub, 0xA405, 1u << JX_SHORT, v);
	if (!have) have = jx_find(T, ifd0, 0xA405, 1u << JX_SHORT, v);
	if (have) X.focal35 = (int)v;
}

inline int jx_exif(const unsigned char* f, int64_t size, JxExif& X) {
	static const unsigned char magic[6] = {0x45, 0x78, 0x69, 0x66, 0x00, 0x00};
	X = JxExif();
	if (!f || size < 4 || f[0] != 0xFF || f[1] != 0xD8) return JX_INVALID;      // jd_parse's "no SOI"
	int64_t pos = 2;
	for (;;) {
		if (pos + 2 > size || f[pos] != 0xFF) return JX_OK;
		const int m = f[pos + 1];
		if (m == 0xFF) { ++pos; continue; }
		if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { pos += 2; continue; }
		if (m == 0xD9 || m == 0xD8 || m == 0x00 || m == 0xDA) return JX_OK;
		if (pos + 4 > size) return JX_OK;
		const int64_t L = (int64_t)f[pos + 2] << 8 | f[pos + 3];
		if (L < 2 || pos + 2 + L > size) return JX_OK;
		const int64_t n = L - 2;
		if (m == 0xE1 && n >= 14 && !memcmp(f + pos + 4, magic, 6)) {
			jx_tiff(f + pos + 10, n - 6, X);
			return JX_OK;
		}
		pos += 2 + L;
	}
}
