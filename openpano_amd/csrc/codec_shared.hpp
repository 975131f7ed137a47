// codec_shared.hpp -- the plumbing the codecs share (png.hip, jpeg.hip, jpeg_dec.hip): source bytes,
// the workgroup prefix sum, the LDS bit writer and the pack kernels' offsets on the device; the file handle, the staging of
// host pixels and the tail of an encode on the host.  A new codec starts from here, not from a copy of a neighbour.
#pragma once
#include "internal.hpp"
#include <cstring>

// byte i of a source image: the fp32 canvas quantised as write_rgb does it, or the byte itself
__device__ __forceinline__ int sample_byte(const float* p, long long i) { return (int)canvas_byte(p[i]); }
__device__ __forceinline__ int sample_byte(const unsigned char* p, long long i) { return (int)p[i]; }

// inclusive prefix sum of a[0..N) in LDS by a workgroup of N threads, t = threadIdx.x.  The caller puts a barrier between its
// own stores to a[] and the call; the sums are visible to every thread on return.
template <int N>
__device__ __forceinline__ void wg_scan_inclusive(uint32_t* a, int t) {
	for (int off = 1; off < N; off <<= 1) {
		const uint32_t v = t >= off ? a[t - off] : 0;
		__syncthreads();
		a[t] += v;
		__syncthreads();
	}
}

// Bit writer into LDS words, one per thread, each starting at any bit offset of one shared image.  The contract of both
// orders: the words are zeroed (and a barrier passed) before the first put; neighbouring writers share the words at their
// seams, so every store is an atomicOr and v must be below 2^nb; at most 31 bits wait in acc between calls.
//   LSB first (deflate): bit k of the stream is bit k % 32 of word k / 32.  put() shifts v up by n <= 31 into the 64-bit
//     accumulator, so nb <= 32 (31 + 32 bits fit, and one word out leaves n <= 31 again); nb = 0 is allowed.
//   MSB first (JPEG): a word is four file bytes, big-endian.  put() shifts the n <= 31 waiting bits up by nb, so nb <= 32
//     by the same sum; the longest put of a baseline JPEG is 27 (a 16-bit code and 11 value bits).
template <bool MSB_FIRST>
struct LdsBitWriter {
	uint32_t* w; unsigned long long acc; int n;
	__device__ __forceinline__ void init(uint32_t* base, uint32_t bitoff) { w = base + (bitoff >> 5); acc = 0; n = (int)(bitoff & 31); }
	__device__ __forceinline__ void put(uint32_t v, int nb) {
		if constexpr (MSB_FIRST) {
			acc = acc << nb | v; n += nb;
			if (n >= 32) { n -= 32; atomicOr(w++, (uint32_t)(acc >> n)); acc &= (1ull << n) - 1; }
		} else {
			acc |= (unsigned long long)v << n; n += nb;
			if (n >= 32) { atomicOr(w++, (uint32_t)acc); acc >>= 32; n -= 32; }
		}
	}
	__device__ __forceinline__ void flush() { if (n > 0) atomicOr(w, MSB_FIRST ? (uint32_t)(acc << (32 - n)) : (uint32_t)acc); }
};
using LsbWriter = LdsBitWriter<false>; using MsbWriter = LdsBitWriter<true>;

// Where slot `slot` of a pack kernel lands: an exclusive scan of the slot sizes, each with `overhead` bytes of framing, done by
// every workgroup (256 threads) for itself -- it sums what lies before its own slot.  offs: a __shared__ word that thread 0
// zeroed before the call (the first of the two barriers here covers that and whatever else the kernel initialises); it holds
// the offset on return.  Not returned by value: a kernel that reads offs where it needs it compiles to the code it always had.
__device__ __forceinline__ void wg_slot_offset(unsigned long long& offs, const uint32_t* __restrict__ sizes, int slot, unsigned long long overhead) {
	__syncthreads();
	unsigned long long part = 0;
	for (int k = threadIdx.x; k < slot; k += 256) part += overhead + sizes[k];
	if (part) atomicAdd(&offs, part);
	__syncthreads();
}

// an encoded file in host memory: what op_png and op_jpeg are
struct EncodedFile { std::vector<unsigned char> bytes; };
inline int64_t encoded_size(const EncodedFile* p) { return p ? (int64_t)p->bytes.size() : 0; }
inline int encoded_copy(const char* who, const EncodedFile* p, unsigned char* host) {
	if (!p || !host) OP_FAIL(OP_ERR_INVALID, std::string(who) + ": bad argument");
	memcpy(host, p->bytes.data(), p->bytes.size());
	return OP_OK;
}

// the *_encode_u8 entry points: h x w x 3 host bytes into a block of the call's, on ctx->stream
inline int stage_rgb_u8(op_ctx* ctx, CallBlocks& own, const unsigned char* rgb_host, int h, int w, unsigned char** d) {
	const size_t n = (size_t)h * w * 3;
	HIPCHK(own.alloc(d, n));
	HIPCHK(hipMemcpyAsync(*d, rgb_host, n, hipMemcpyHostToDevice, ctx->stream));
	return OP_OK;
}

// The tail of an encode.  The pack kernel left *total bytes at obuf; they are appended to what already stands in file.bytes (nothing
// for PNG, the host's header for JPEG).  least / cap: the fewest and the most the kernels can have written.  The call's one wait is here.
inline int encoded_fetch(op_ctx* ctx, CallBlocks& own, const unsigned char* obuf, const unsigned long long* total, size_t least, size_t cap, EncodedFile& file, const char* label, const char* who) {
	hipStream_t st = ctx->stream;
	unsigned long long n = 0;
	HIPCHK(hipMemcpyAsync(&n, total, sizeof(n), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	if (n < least || n > cap) OP_FAIL(OP_ERR_HIP, std::string(who) + ": the device reported an impossible file size");
	const size_t head = file.bytes.size();
	file.bytes.resize(head + (size_t)n);
	{ ProfScope ps(ctx, label);
	  HIPCHK(hipMemcpyAsync(file.bytes.data() + head, obuf, (size_t)n, hipMemcpyDeviceToHost, st)); }
	HIPCHK(own.finish());
	resolve_profile(ctx);
	return OP_OK;
}
