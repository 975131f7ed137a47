// jpeg.hip -- the canvas as a baseline JPEG file, encoded on the device.
//
// Stands in for write_rgb -> CImg::save_jpeg -> libjpeg (lib/imgio.cc:98-113, called by main.cc:30,233): sequential DCT,
// 8 bits, 4:4:4 or 4:2:0, the Huffman tables of ITU T.81 Annex K.3, a restart marker every OP_JPEG_RI_444 / OP_JPEG_RI_420
// MCUs.  A restart interval is byte-aligned and starts its DC prediction at 0, so intervals are independent.  Two kernels:
//   k_jpeg_interval  one workgroup per restart interval: quantise the canvas (canvas_byte), RGB -> YCbCr,
//                    4:2:0 chroma averaging, IJG slow-integer forward DCT (rows, then columns), quantisation, zigzag -- all in
//                    LDS; one thread per block counts its bits, a prefix sum (wg_scan_inclusive) places them, MsbWriter ORs the codes
//                    into an LDS bit image, a second prefix sum (of 0xFF bytes) places the stuffed bytes in the interval's slot;
//   k_jpeg_pack      exclusive scan of the slot sizes (wg_slot_offset), every interval copied to its place behind the header,
//                    RSTn between them, EOI at the end.  (These helpers, sample_byte and the file handle: codec_shared.hpp.)
// The header (SOI .. SOS, 623 bytes) is written by the host.  All arithmetic after the byte quantisation is integer and the
// only atomics are integer OR / add on LDS, so the file is a function of the pixels alone; tests/harness/jpeg_ref.c is the same
// encoder written serially, its files equal libjpeg's byte for byte, and the GPU tests require the device's to equal its.
#include "codec_shared.hpp"
#include "jpeg_tables.hpp"

// MCUs per restart interval (8 x 8 pixels at 4:4:4, 16 x 16 at 4:2:0); tests/harness/jpeg_ref.c has the same knobs
#ifndef OP_JPEG_RI_444
#define OP_JPEG_RI_444 32
#endif
#ifndef OP_JPEG_RI_420
#define OP_JPEG_RI_420 8
#endif
#define JPEG_BLOCK_BYTES 208        // worst case of one block: 20 + 63 * 26 bits
#define JPEG_WS 72                  // ints of DCT workspace per block: rows of 9, so row and column passes are free of bank conflicts
#define JPEG_ZS 66                  // shorts per block of zigzagged coefficients: 33 words, one bank apart per thread
static_assert(OP_JPEG_RI_444 >= 1 && OP_JPEG_RI_444 * 3 <= 256 && OP_JPEG_RI_420 >= 1 && OP_JPEG_RI_420 * 6 <= 256, "one thread codes one block");

struct op_jpeg : EncodedFile {};

namespace {

// the quantiser bases and the zigzag order (the header's DQT segments) are jpeg_tables.hpp's, shared with the decoder
__constant__ unsigned char c_k1[64] = JPEG_K1_LUMA, c_k2[64] = JPEG_K2_CHROMA;
const unsigned char h_k1[64] = JPEG_K1_LUMA, h_k2[64] = JPEG_K2_CHROMA, h_zigzag[64] = JPEG_ZZ_NAT;
// natural index -> zigzag position: the inverse of JPEG_ZZ_NAT
#define JPEG_ZZ_POS {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, \
	10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63}
__constant__ unsigned char c_zz_pos[64] = JPEG_ZZ_POS;
static_assert([] { constexpr unsigned char pos[64] = JPEG_ZZ_POS, nat[64] = JPEG_ZZ_NAT; for (int k = 0; k < 64; ++k) if (pos[nat[k]] != k) return false; return true; }(),
	"c_zz_pos must send every natural index to its place in the one zigzag order");

// ITU T.81 Annex K.3: code counts per length 1..16 and the symbols in code order; index 0 luma, 1 chroma
#define JPEG_DC_COUNTS {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}}
#define JPEG_AC_COUNTS {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}}
#define JPEG_AC_VALS {{ \
	1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, \
	130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, \
	90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, \
	150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, \
	199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, \
	246, 247, 248, 249, 250}, { \
	0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, \
	10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, \
	89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, \
	148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, \
	197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, \
	246, 247, 248, 249, 250}}
__constant__ unsigned char c_dc_counts[2][16] = JPEG_DC_COUNTS;
__constant__ unsigned char c_ac_counts[2][16] = JPEG_AC_COUNTS;
__constant__ unsigned char c_ac_vals[2][162] = JPEG_AC_VALS;
const unsigned char h_dc_counts[2][16] = JPEG_DC_COUNTS;
const unsigned char h_ac_counts[2][16] = JPEG_AC_COUNTS;
const unsigned char h_ac_vals[2][162] = JPEG_AC_VALS;

__host__ __device__ inline int jpeg_q(int base, int quality) {
	const int S = quality < 50 ? 5000 / quality : 200 - 2 * quality;
	const int v = (base * S + 50) / 100;
	return v < 1 ? 1 : v > 255 ? 255 : v;
}

template <typename T>
__device__ __forceinline__ void load_ycc(const T* __restrict__ src, int w, int y, int x, int& Y, int& Cb, int& Cr) {
	const long long i = 3 * ((long long)y * w + x);
	const int R = sample_byte(src, i), G = sample_byte(src, i + 1), B = sample_byte(src, i + 2);
	Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
	Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
	Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the IJG slow-integer forward DCT (13-bit constants, 2 bits of headroom kept by the row pass) over eight
// values STRIDE ints apart; every index is a compile-time constant, so the eight values live in registers
template <int STRIDE, bool COLUMNS>
__device__ __forceinline__ void fdct_pass(const int* d, int (&o)[8]) {
	const int d0 = d[0], d1 = d[STRIDE], d2 = d[2 * STRIDE], d3 = d[3 * STRIDE], d4 = d[4 * STRIDE], d5 = d[5 * STRIDE], d6 = d[6 * STRIDE], d7 = d[7 * STRIDE];
	const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
	const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
	constexpr int s = COLUMNS ? 15 : 11;
	o[0] = COLUMNS ? descale(t10 + t11, 2) : (t10 + t11) * 4;
	o[4] = COLUMNS ? descale(t10 - t11, 2) : (t10 - t11) * 4;
	const int z = (t12 + t13) * 4433;
	o[2] = descale(z + t13 * 6270, s);
	o[6] = descale(z - t12 * 15137, s);
	const int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
	const int y3 = z5 - z3 * 16069, y4 = z5 - z4 * 3196;
	o[7] = descale(t4 * 2446 - z1 * 7373 + y3, s);
	o[5] = descale(t5 * 16819 - z2 * 20995 + y4, s);
	o[3] = descale(t6 * 25172 - z2 * 20995 + y3, s);
	o[1] = descale(t7 * 12299 - z1 * 7373 + y4, s);
}

// k-th symbol (in code order) of a table with these counts: its canonical code and length
__device__ __forceinline__ uint32_t huff_entry(const unsigned char* counts, int k) {
	uint32_t code = 0; int base = 0;
	for (int len = 1; len <= 16; ++len) {
		const int n = counts[len - 1];
		if (k < base + n) return (code + (uint32_t)(k - base)) << 5 | (uint32_t)len;
		code = (code + (uint32_t)n) << 1; base += n;
	}
	return 0;
}

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v); }      // v >= 0

// Huffman entry = code << 5 | length.  EMIT = false: only the block's length in bits is returned.  No put exceeds 16 + 11 bits.
template <bool EMIT>
__device__ __forceinline__ uint32_t code_block(const short* zz, int pred, const uint32_t* hdc, const uint32_t* hac, MsbWriter& bw) {
	uint32_t bits = 0;
	{
		const int d = (int)zz[0] - pred, cat = bit_length(d < 0 ? -d : d);
		const uint32_t e = hdc[cat], len = e & 31;
		bits += len + cat;
		if (EMIT) bw.put((e >> 5) << cat | ((uint32_t)(d > 0 ? d : d - 1) & ((1u << cat) - 1)), (int)len + cat);
	}
	int run = 0;
	for (int k = 1; k < 64; ++k) {
		const int v = zz[k];
		if (!v) { ++run; continue; }
		while (run >= 16) { const uint32_t e = hac[0xF0]; bits += e & 31; if (EMIT) bw.put(e >> 5, (int)(e & 31)); run -= 16; }
		const int cat = bit_length(v < 0 ? -v : v);
		const uint32_t e = hac[run << 4 | cat], len = e & 31;
		bits += len + cat;
		if (EMIT) bw.put((e >> 5) << cat | ((uint32_t)(v > 0 ? v : v - 1) & ((1u << cat) - 1)), (int)len + cat);
		run = 0;
	}
	if (run) { const uint32_t e = hac[0]; bits += e & 31; if (EMIT) bw.put(e >> 5, (int)(e & 31)); }
	return bits;
}

template <int MODE> struct JpegGeom;
template <> struct JpegGeom<OP_JPEG_444> { static constexpr int RI = OP_JPEG_RI_444, BPM = 3; };
template <> struct JpegGeom<OP_JPEG_420> { static constexpr int RI = OP_JPEG_RI_420, BPM = 6; };

template <int MODE>
struct JpegLds {
	static constexpr int NB = JpegGeom<MODE>::RI * JpegGeom<MODE>::BPM;
	union { int ws[NB * JPEG_WS]; uint32_t bits[NB * JPEG_BLOCK_BYTES / 4]; } u;      // the workspace is dead before the bit image is cleared
	short zz[NB * JPEG_ZS];
	uint32_t hdc[2][16], hac[2][256];
	uint32_t scan[256];
	unsigned short q8[2][64];       // 8 * Q, natural order
	unsigned char zzpos[64];
	unsigned char dummy[NB];
	short mcu_y[JpegGeom<MODE>::RI], mcu_x[JpegGeom<MODE>::RI];
};

// slots: nint x SLOT bytes, SLOT = 2 * NB * 208 (every block at its worst, every byte stuffed); sizes: bytes used per slot
template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_jpeg_interval(const T* __restrict__ src, int h, int w, int quality, int mw, long long nmcu,
		unsigned char* __restrict__ slots, uint32_t* __restrict__ sizes) {
	using G = JpegGeom<MODE>;
	constexpr int NB = JpegLds<MODE>::NB, BPM = G::BPM;
	__shared__ JpegLds<MODE> S;
	const int t = threadIdx.x;
	const long long m0 = (long long)blockIdx.x * G::RI;
	const int nm = (int)(nmcu - m0 < G::RI ? nmcu - m0 : G::RI), nblk = nm * BPM;

	// ---- tables: quantisers, zigzag, the four Huffman tables; where this interval's MCUs are; which Y blocks are dummies
	if (t < 128) { const int k = t & 63; S.q8[t >> 6][k] = (unsigned short)(8 * jpeg_q(t < 64 ? c_k1[k] : c_k2[k], quality)); }
	if (t < 64) S.zzpos[t] = c_zz_pos[t];
	for (int k = t; k < 512; k += 256) S.hac[k >> 8][k & 255] = 0;
	if (t < 32) S.hdc[t >> 4][t & 15] = 0;
	__syncthreads();
	if (t < 162) { S.hac[0][c_ac_vals[0][t]] = huff_entry(c_ac_counts[0], t); S.hac[1][c_ac_vals[1][t]] = huff_entry(c_ac_counts[1], t); }
	if (t < 12) { S.hdc[0][t] = huff_entry(c_dc_counts[0], t); S.hdc[1][t] = huff_entry(c_dc_counts[1], t); }
	if (t < nm) {
		const long long m = m0 + t;
		const int my = (int)(m / mw), mx = (int)(m - (long long)my * mw);
		S.mcu_y[t] = (short)my; S.mcu_x[t] = (short)mx;
		if (MODE == OP_JPEG_420) {
			const int bw8 = (w + 7) >> 3, bh8 = (h + 7) >> 3;
			for (int k = 0; k < 6; ++k) S.dummy[t * 6 + k] = (k < 4 && (mx * 2 + (k & 1) >= bw8 || my * 2 + (k >> 1) >= bh8)) ? 1 : 0;
		} else {
			for (int k = 0; k < 3; ++k) S.dummy[t * 3 + k] = 0;
		}
	}
	__syncthreads();

	// ---- samples - 128 into the workspace; edges repeat
	if (MODE == OP_JPEG_444) {
		for (int p = t; p < nm * 64; p += 256) {
			const int mcu = p >> 6, yy = (p >> 3) & 7, xx = p & 7;
			const int y = min(S.mcu_y[mcu] * 8 + yy, h - 1), x = min(S.mcu_x[mcu] * 8 + xx, w - 1);
			int Y, Cb, Cr;
			load_ycc(src, w, y, x, Y, Cb, Cr);
			int* o = S.u.ws + mcu * 3 * JPEG_WS + yy * 9 + xx;
			o[0] = Y - 128; o[JPEG_WS] = Cb - 128; o[2 * JPEG_WS] = Cr - 128;
		}
	} else {
		// one 2 x 2 cell per task: four Y samples and one Cb / Cr average.  Chroma pads the full-resolution rows to an even
		// count only and repeats DOWNSAMPLED rows below that, so under the last chroma row a cell's chroma comes from other
		// rows than its Y (which repeats the last image row).
		const int ch = (h + 1) >> 1;
		for (int p = t; p < nm * 64; p += 256) {
			const int mcu = p >> 6, cyl = (p >> 3) & 7, cxl = p & 7;
			const int cy = S.mcu_y[mcu] * 8 + cyl, cx = S.mcu_x[mcu] * 8 + cxl, cyc = min(cy, ch - 1);
			const int blk = mcu * 6 + ((cyl >> 2) << 1 | (cxl >> 2));
			const bool real = !S.dummy[blk];
			int* oy = S.u.ws + blk * JPEG_WS + ((2 * cyl) & 7) * 9 + ((2 * cxl) & 7);
			int sb = 0, sr = 0;
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int x = min(2 * cx + (j & 1), w - 1);
				int Y, Cb, Cr;
				load_ycc(src, w, min(2 * cy + (j >> 1), h - 1), x, Y, Cb, Cr);
				if (real) oy[(j >> 1) * 9 + (j & 1)] = Y - 128;
				if (cyc != cy) load_ycc(src, w, min(2 * cyc + (j >> 1), h - 1), x, Y, Cb, Cr);
				sb += Cb; sr += Cr;
			}
			const int bias = (cx & 1) ? 2 : 1;
			int* oc = S.u.ws + (mcu * 6 + 4) * JPEG_WS + cyl * 9 + cxl;
			oc[0] = ((sb + bias) >> 2) - 128; oc[JPEG_WS] = ((sr + bias) >> 2) - 128;
		}
	}
	__syncthreads();

	// ---- forward DCT: one thread per row of a block, then one per column; quantised and zigzagged on the way out
	for (int i = t; i < nblk * 8; i += 256) {
		const int b = i >> 3, r = i & 7;
		if (S.dummy[b]) continue;
		int* d = S.u.ws + b * JPEG_WS + r * 9;
		int o[8];
		fdct_pass<1, false>(d, o);
#pragma unroll
		for (int k = 0; k < 8; ++k) d[k] = o[k];
	}
	__syncthreads();
	for (int i = t; i < nblk * 8; i += 256) {
		const int b = i >> 3, c = i & 7;
		if (S.dummy[b]) continue;
		const int tq = (b % BPM) >= (MODE == OP_JPEG_420 ? 4 : 1) ? 1 : 0;
		int o[8];
		fdct_pass<9, true>(S.u.ws + b * JPEG_WS + c, o);
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const int nat = k * 8 + c, qv = S.q8[tq][nat], v = o[k];
			const int a = ((v < 0 ? -v : v) + (qv >> 1)) / qv;
			S.zz[b * JPEG_ZS + S.zzpos[nat]] = (short)(v < 0 ? -a : a);
		}
	}
	__syncthreads();

	// ---- the workspace is dead: clear the bit image over it; one thread per block counts its bits
	for (int k = t; k < NB * JPEG_BLOCK_BYTES / 4; k += 256) S.u.bits[k] = 0;
	const int b = t;
	const bool coding = b < nblk, dummy = coding && S.dummy[b];
	const int comp = b % BPM, tq = comp >= (MODE == OP_JPEG_420 ? 4 : 1) ? 1 : 0;
	int pred = 0;
	uint32_t mybits = 0;
	MsbWriter bw = {nullptr, 0, 0};
	if (coding && !dummy) {
		// the previous block of the same component inside the interval; a dummy Y block repeats the DC before it, so it is skipped
		if (MODE == OP_JPEG_444 || comp >= 4) { if (b >= BPM) pred = S.zz[(b - BPM) * JPEG_ZS]; }
		else {
			for (int pb = b;;) {
				pb = (pb % 6) ? pb - 1 : pb - 3;
				if (pb < 0) break;
				if (!S.dummy[pb]) { pred = S.zz[pb * JPEG_ZS]; break; }
			}
		}
		mybits = code_block<false>(S.zz + b * JPEG_ZS, pred, S.hdc[tq], S.hac[tq], bw);
	} else if (dummy) mybits = (S.hdc[0][0] & 31) + (S.hac[0][0] & 31);      // DC difference 0, end of block
	S.scan[t] = mybits;
	__syncthreads();
	wg_scan_inclusive<256>(S.scan, t);
	const uint32_t total = S.scan[255];
	if (coding) {
		bw.init(S.u.bits, S.scan[t] - mybits);
		if (dummy) { bw.put(S.hdc[0][0] >> 5, (int)(S.hdc[0][0] & 31)); bw.put(S.hac[0][0] >> 5, (int)(S.hac[0][0] & 31)); }
		else code_block<true>(S.zz + b * JPEG_ZS, pred, S.hdc[tq], S.hac[tq], bw);
		bw.flush();
	}
	const int pad = (int)(-total & 7);
	if (t == 0 && pad) atomicOr(&S.u.bits[total >> 5], ((1u << pad) - 1) << (32 - (int)(total & 31) - pad));      // 1-bits up to the byte
	__syncthreads();

	// ---- byte stuffing: a thread owns a run of bytes; the 0xFF bytes before the run say where it lands
	const uint32_t nbytes = (total + 7) >> 3, chunk = (nbytes + 255) / 256;
	const uint32_t i0 = min((uint32_t)t * chunk, nbytes), i1 = min(i0 + chunk, nbytes);
	uint32_t ff = 0;
	for (uint32_t i = i0; i < i1; ++i) ff += ((S.u.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255) == 255 ? 1 : 0;
	__syncthreads();
	S.scan[t] = ff;
	__syncthreads();
	wg_scan_inclusive<256>(S.scan, t);
	unsigned char* slot = slots + (long long)blockIdx.x * (2 * NB * JPEG_BLOCK_BYTES);
	uint32_t o = i0 + S.scan[t] - ff;
	for (uint32_t i = i0; i < i1; ++i) {
		const uint32_t v = (S.u.bits[i >> 2] >> (24 - 8 * (i & 3))) & 255;
		slot[o++] = (unsigned char)v;
		if (v == 255) slot[o++] = 0;
	}
	if (t == 0) sizes[blockIdx.x] = nbytes + S.scan[255];
}

// out: the entropy-coded data and EOI (the header is the host's); *total = their length
__global__ void __launch_bounds__(256) k_jpeg_pack(const unsigned char* __restrict__ slots, const uint32_t* __restrict__ sizes, int slot_bytes,
		int nint, unsigned char* __restrict__ out, unsigned long long* __restrict__ total) {
	__shared__ unsigned long long offs;
	const int t = threadIdx.x, iv = blockIdx.x;
	if (t == 0) offs = 0;
	wg_slot_offset(offs, sizes, iv, 2);      // each interval is followed by a 2-byte marker
	const uint32_t size = sizes[iv];
	unsigned char* o = out + offs;
	const unsigned char* slot = slots + (long long)iv * slot_bytes;
	for (uint32_t j = t; j < size; j += 256) o[j] = slot[j];
	if (t == 0) {
		o[size] = 0xFF;
		o[size + 1] = iv == nint - 1 ? 0xD9 : (unsigned char)(0xD0 + (iv & 7));      // EOI, or RSTn
		if (iv == nint - 1) *total = offs + size + 2;
	}
}

void put16(std::vector<unsigned char>& o, int v) { o.push_back((unsigned char)(v >> 8)); o.push_back((unsigned char)v); }

// SOI, APP0 (JFIF 1.1, density 1 x 1, no unit), DQT luma, DQT chroma, SOF0, DHT DC0 AC0 DC1 AC1, DRI, SOS
std::vector<unsigned char> jpeg_header(int h, int w, int quality, int subsampling) {
	std::vector<unsigned char> o = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
	for (int t = 0; t < 2; ++t) {
		o.push_back(0xFF); o.push_back(0xDB); put16(o, 67); o.push_back((unsigned char)t);
		for (int k = 0; k < 64; ++k) o.push_back((unsigned char)jpeg_q((t ? h_k2 : h_k1)[h_zigzag[k]], quality));
	}
	o.push_back(0xFF); o.push_back(0xC0); put16(o, 17); o.push_back(8); put16(o, h); put16(o, w); o.push_back(3);
	for (int c = 0; c < 3; ++c) { o.push_back((unsigned char)(c + 1)); o.push_back(c == 0 && subsampling == OP_JPEG_420 ? 0x22 : 0x11); o.push_back(c ? 1 : 0); }
	for (int t = 0; t < 4; ++t) {
		const int cls = t & 1, id = t >> 1, nv = cls ? 162 : 12;
		o.push_back(0xFF); o.push_back(0xC4); put16(o, 2 + 1 + 16 + nv); o.push_back((unsigned char)(cls << 4 | id));
		for (int k = 0; k < 16; ++k) o.push_back(cls ? h_ac_counts[id][k] : h_dc_counts[id][k]);
		for (int k = 0; k < nv; ++k) o.push_back(cls ? h_ac_vals[id][k] : (unsigned char)k);
	}
	o.push_back(0xFF); o.push_back(0xDD); put16(o, 4); put16(o, subsampling == OP_JPEG_420 ? OP_JPEG_RI_420 : OP_JPEG_RI_444);
	const unsigned char sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
	o.insert(o.end(), sos, sos + sizeof sos);
	return o;
}

template <typename T, int MODE>
void launch_interval(const void* src, int h, int w, int quality, int mw, long long nmcu, int nint, unsigned char* slots, uint32_t* sizes, hipStream_t st) {
	hipLaunchKernelGGL((k_jpeg_interval<T, MODE>), dim3(nint), dim3(256), 0, st, (const T*)src, h, w, quality, mw, nmcu, slots, sizes);
}

int check_args(int h, int w, int quality, int subsampling, const char* who) {
	if (quality < 1 || quality > 100) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": quality outside 1..100");
	if (subsampling != OP_JPEG_444 && subsampling != OP_JPEG_420) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": unknown subsampling (OP_JPEG_444 or OP_JPEG_420)");
	if (h < 1 || w < 1) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": empty image (h = 0 or w = 0): a JPEG cannot hold a zero-sized image");
	if (h > 65535 || w > 65535) OP_FAIL(OP_ERR_UNSUPPORTED, std::string(who) + ": a JPEG frame header holds 16-bit dimensions (h, w <= 65535)");
	return OP_OK;
}

// src: device H x W x 3, fp32 canvas or bytes; own: the call's blocks (on ctx->stream); the arguments have passed check_args
int encode_device(op_ctx* ctx, CallBlocks& own, const void* src, bool is_float, int h, int w, int quality, int subsampling, op_jpeg** out, const char* who) {
	const bool s420 = subsampling == OP_JPEG_420;
	const int mcu = s420 ? 16 : 8, ri = s420 ? OP_JPEG_RI_420 : OP_JPEG_RI_444, bpm = s420 ? 6 : 3;
	const int mw = (w + mcu - 1) / mcu, mh = (h + mcu - 1) / mcu;
	const long long nmcu = (long long)mw * mh;
	const int nint = (int)((nmcu + ri - 1) / ri);
	const int slot_bytes = 2 * ri * bpm * JPEG_BLOCK_BYTES;
	const size_t cap = (size_t)nint * ((size_t)slot_bytes + 2);
	hipStream_t st = ctx->stream;
	unsigned char *slots = nullptr, *obuf = nullptr; uint32_t* sizes = nullptr; unsigned long long* total = nullptr;
	HIPCHK(own.alloc(&slots, (size_t)nint * slot_bytes));
	HIPCHK(own.alloc(&sizes, sizeof(uint32_t) * (size_t)nint));
	HIPCHK(own.alloc(&obuf, cap));
	HIPCHK(own.alloc(&total, sizeof(unsigned long long)));
	{ ProfScope ps(ctx, "jpeg interval");
	  if (is_float) { if (s420) launch_interval<float, OP_JPEG_420>(src, h, w, quality, mw, nmcu, nint, slots, sizes, st); else launch_interval<float, OP_JPEG_444>(src, h, w, quality, mw, nmcu, nint, slots, sizes, st); }
	  else { if (s420) launch_interval<unsigned char, OP_JPEG_420>(src, h, w, quality, mw, nmcu, nint, slots, sizes, st); else launch_interval<unsigned char, OP_JPEG_444>(src, h, w, quality, mw, nmcu, nint, slots, sizes, st); }
	  HIPCHK(hipGetLastError()); }
	{ ProfScope ps(ctx, "jpeg pack");
	  hipLaunchKernelGGL(k_jpeg_pack, dim3(nint), dim3(256), 0, st, slots, sizes, slot_bytes, nint, obuf, total);
	  HIPCHK(hipGetLastError()); }
	std::unique_ptr<op_jpeg> jpg(new op_jpeg);
	jpg->bytes = jpeg_header(h, w, quality, subsampling);
	if (const int r = encoded_fetch(ctx, own, obuf, total, 3, cap, *jpg, "jpeg D2H", who)) return r;      // at least one byte and EOI
	*out = jpg.release();
	return OP_OK;
}

}	// namespace

extern "C" {

int op_canvas_encode_jpeg(op_ctx* ctx, const op_canvas* c, int quality, int subsampling, op_jpeg** out) {
	if (!ctx || !c || !out) OP_FAIL(OP_ERR_INVALID, "op_canvas_encode_jpeg: bad argument");
	int h = 0, w = 0;
	if (op_canvas_dims(c, &h, &w) != OP_OK) return OP_ERR_INVALID;
	if (const int r = check_args(h, w, quality, subsampling, "op_canvas_encode_jpeg")) return r;
	HIPCHK(hipSetDevice(ctx->device));
	CallBlocks own({ctx->stream});
	return encode_device(ctx, own, op_canvas_device(c), true, h, w, quality, subsampling, out, "op_canvas_encode_jpeg");
}

int op_jpeg_encode_u8(op_ctx* ctx, const unsigned char* rgb_host, int h, int w, int quality, int subsampling, op_jpeg** out) {
	if (!ctx || !rgb_host || !out) OP_FAIL(OP_ERR_INVALID, "op_jpeg_encode_u8: bad argument");
	if (const int r = check_args(h, w, quality, subsampling, "op_jpeg_encode_u8")) return r;
	HIPCHK(hipSetDevice(ctx->device));
	CallBlocks own({ctx->stream});
	unsigned char* d = nullptr;
	if (const int r = stage_rgb_u8(ctx, own, rgb_host, h, w, &d)) return r;
	return encode_device(ctx, own, d, false, h, w, quality, subsampling, out, "op_jpeg_encode_u8");
}

int64_t op_jpeg_size(const op_jpeg* p) { return encoded_size(p); }
int op_jpeg_copy(op_ctx*, const op_jpeg* p, unsigned char* host) { return encoded_copy("op_jpeg_copy", p, host); }

void op_jpeg_free(op_jpeg* p) { delete p; }

}	// extern "C"
