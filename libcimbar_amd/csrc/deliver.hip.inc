// deliver.hip.inc -- part of cimbar_hip.hip: chunk delivery (cimbar_hip_deliver_chunks / _delivery_reset / _delivery_stats). Included ONCE, in front
// of the per-mode copies: nothing here depends on the grid beyond three integers (frames, chunks per frame, chunk size).
//
// A batch's fixed slots + one mask word per frame -> the delivered chunks packed front to back in frame and slot order (escrow_buffer_writer per
// frame, concatenated: what cimbard_fountain_decode walks), optionally without the chunks a fountain_decoder_sink refuses anyway: a header that
// says file size 0 (decode_frame returns -11) and a 6-byte header it has seen before (FountainDecoder::decode's std::set of block ids).
//   D1 k_deliver_mark    one lane per (frame, slot): mask bit, six header bytes, DROP_EMPTY; DEDUP: claim the 48-bit key in the call's scratch
//                        table (64-bit atomicCAS) and atomicMin the candidate index beside it
//   D2 k_deliver_select  one lane per (frame, slot): kept <=> the candidate IS that minimum, and (REMEMBER) its key is not in the context's table
//                        (read-only lookup) -> one bit of the frame's kept word
//   D3 k_deliver_scan    one workgroup: exclusive scan of popcount(kept) over the frames -> per-frame output base, count, the REMEMBER decision
//   D4 k_deliver_copy    one wavefront per kept chunk: src[k], the copy (source and destination each arbitrary modulo 4), the insert into the
//                        context's table where D3 allowed it
// The output depends on the inputs and the remembered SET alone: which lane claims a scratch entry first changes where a key lies, never the
// minimum recorded beside it; the persistent table is only ever asked "is this key in it".
namespace deliver __attribute__((visibility("hidden"))) {

namespace {

constexpr unsigned long long KEY_TAG = 1ull << 63;   // every stored key carries it, so that 0 means "free entry" (a header of six zero bytes is a key like any other)
constexpr int DEFAULT_CAP_LOG2 = 20, MIN_CAP_LOG2 = 4, MAX_CAP_LOG2 = 24;
constexpr int MAX_SLOTS = 1 << 24;                   // frames * chunks per frame of one call (the scratch table then has 2^25 entries)
constexpr unsigned ALL_FLAGS = CIMBAR_HIP_DELIVER_DEDUP | CIMBAR_HIP_DELIVER_REMEMBER | CIMBAR_HIP_DELIVER_DROP_EMPTY;

struct Ctl {                 // device-resident, owned by the context
	uint32_t remembered;     // keys in the persistent table
	uint32_t overflowed;     // sticky: a REMEMBER call could not record its headers
	uint32_t insert;         // D3's decision for the call in flight: D4 records the kept headers
	uint32_t pad;
};

// murmur3's 64-bit finaliser: block ids count up in the low bytes, the table wants them spread
__device__ __forceinline__ uint32_t key_hash(unsigned long long k)
{
	k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
	k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
	k ^= k >> 33;
	return (uint32_t)k;
}

// D1. `where[i]`: -1 = not a candidate, else the scratch-table entry of its key (0 without DEDUP)
__global__ __launch_bounds__(256) void k_deliver_mark(const uint8_t* __restrict__ chunks, const uint32_t* __restrict__ masks, int total, int per, int cs,
                                                      unsigned flags, unsigned long long* __restrict__ keys, uint32_t* __restrict__ first, uint32_t tmask,
                                                      int32_t* __restrict__ where)
{
	const int i = (int)(blockIdx.x * 256u + threadIdx.x);
	if (i >= total) return;
	const int f = i / per, s = i - f * per;
	int32_t w = -1;
	if ((masks[f] >> s) & 1u) {
		// slots start at slot * 625 and the like: byte loads, no alignment assumed
		const uint8_t* h = chunks + (size_t)i * (size_t)cs;
		const uint32_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3], b4 = h[4], b5 = h[5];
		const bool empty = !(b0 & 0x80u) && !(b1 | b2 | b3);   // FountainMetadata::file_size() == 0
		if (!((flags & CIMBAR_HIP_DELIVER_DROP_EMPTY) && empty)) {
			w = 0;
			if (flags & CIMBAR_HIP_DELIVER_DEDUP) {
				const unsigned long long key = KEY_TAG | ((unsigned long long)((b0 << 8) | b1) << 32) | ((b2 << 24) | (b3 << 16) | (b4 << 8) | b5);
				uint32_t e = key_hash(key) & tmask;
				for (;;) {   // the table holds at least twice the candidates: a free entry is always found
					const unsigned long long prev = atomicCAS(&keys[e], 0ull, key);
					if (prev == 0ull || prev == key) break;
					e = (e + 1u) & tmask;
				}
				atomicMin(&first[e], (uint32_t)i);
				w = (int32_t)e;
			}
		}
	}
	where[i] = w;
}

// D2. `kept` is zero on entry
__global__ __launch_bounds__(256) void k_deliver_select(const int32_t* __restrict__ where, int total, int per, unsigned flags,
                                                        const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ first,
                                                        const unsigned long long* __restrict__ table, uint32_t pmask, uint32_t* __restrict__ kept)
{
	const int i = (int)(blockIdx.x * 256u + threadIdx.x);
	if (i >= total) return;
	const int32_t w = where[i];
	bool keep = w >= 0;
	if (keep && (flags & CIMBAR_HIP_DELIVER_DEDUP)) {
		keep = first[w] == (uint32_t)i;
		if (keep && (flags & CIMBAR_HIP_DELIVER_REMEMBER)) {
			const unsigned long long key = keys[w];
			uint32_t e = key_hash(key) & pmask;
			for (;;) {   // at most half full: a free entry ends every probe
				const unsigned long long k = table[e];
				if (k == key) { keep = false; break; }
				if (k == 0ull) break;
				e = (e + 1u) & pmask;
			}
		}
	}
	if (keep) {
		const int f = i / per;
		atomicOr(&kept[f], 1u << (i - f * per));
	}
}

// inclusive sum over the wavefront: four DPP row shifts inside each row of 16, then the three row totals in front
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1 (lanes without a source add 0)
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
	const uint32_t r0 = (uint32_t)__shfl((int)v, 15), r1 = (uint32_t)__shfl((int)v, 31), r2 = (uint32_t)__shfl((int)v, 47);
	const int row = lane >> 4;
	return v + (row > 0 ? r0 : 0u) + (row > 1 ? r1 : 0u) + (row > 2 ? r2 : 0u);
}

// D3. one workgroup of 1024 lanes walks the frames 1024 at a time
__global__ __launch_bounds__(1024) void k_deliver_scan(const uint32_t* __restrict__ kept, int n, uint32_t* __restrict__ base, int32_t* __restrict__ count,
                                                       unsigned flags, Ctl* __restrict__ ctl, uint32_t capacity)
{
	__shared__ uint32_t wsum[16];
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t carry = 0;
	for (int f0 = 0; f0 < n; f0 += 1024) {
		const int f = f0 + tid;
		const uint32_t c = f < n ? (uint32_t)__popc(kept[f]) : 0u;
		const uint32_t incl = wave_inclusive_sum(c, lane);
		if (lane == 63) wsum[wave] = incl;
		__syncthreads();
		uint32_t before = 0, all = 0;
		for (int w = 0; w < 16; ++w) {
			const uint32_t v = wsum[w];
			before += w < wave ? v : 0u;
			all += v;
		}
		if (f < n) base[f] = carry + before + incl - c;
		carry += all;
		__syncthreads();
	}
	if (tid == 0) {
		*count = (int32_t)carry;
		if (flags & CIMBAR_HIP_DELIVER_REMEMBER) {
			// all of the call's new headers or none: the table never passes one half, and a call it cannot take loses nothing -- its chunks are
			// delivered, only not remembered
			const bool fits = ctl->remembered + carry <= capacity / 2u;
			ctl->insert = fits ? 1u : 0u;
			if (fits) ctl->remembered += carry;
			else ctl->overflowed = 1u;
		}
	}
}

// D4. four wavefronts per workgroup, one per linear slot; a wavefront whose slot is not kept leaves at once
__global__ __launch_bounds__(256) void k_deliver_copy(const uint8_t* __restrict__ chunks, const uint32_t* __restrict__ kept, const uint32_t* __restrict__ base,
                                                      int total, int per, int cs, uint8_t* __restrict__ packed, int32_t* __restrict__ src, unsigned flags,
                                                      const int32_t* __restrict__ where, const unsigned long long* __restrict__ keys,
                                                      const Ctl* __restrict__ ctl, unsigned long long* __restrict__ table, uint32_t pmask)
{
	const int i = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
	if (i >= total) return;
	const int f = i / per, s = i - f * per;
	const uint32_t kb = kept[f];
	if (!((kb >> s) & 1u)) return;
	const uint32_t k = base[f] + (uint32_t)__popc(kb & ((1u << s) - 1u));
	if (lane == 0) {
		if (src) src[k] = i;
		if ((flags & CIMBAR_HIP_DELIVER_REMEMBER) && ctl->insert) {
			const unsigned long long key = keys[where[i]];   // kept keys are distinct and none is in the table yet
			uint32_t e = key_hash(key) & pmask;
			while (atomicCAS(&table[e], 0ull, key) != 0ull) e = (e + 1u) & pmask;
		}
	}
	const uint8_t* sp = chunks + (size_t)i * (size_t)cs;
	uint8_t* dp = packed + (size_t)k * (size_t)cs;
	// head bytes up to the destination's first dword boundary, whole destination dwords, tail bytes. A destination dword comes from the one or two
	// ALIGNED source dwords that hold its bytes (each of them holds at least one byte of this chunk: nothing is read that does not share a dword
	// with the chunk, nothing is written outside it)
	const int head = (int)((4u - (unsigned)((uintptr_t)dp & 3u)) & 3u);
	const int nd = (cs - head) >> 2, tail = (cs - head) & 3;
	if (lane < head) dp[lane] = sp[lane];
	const uint8_t* sb = sp + head;
	const unsigned sh = (unsigned)((uintptr_t)sb & 3u);
	const uint32_t* sa = reinterpret_cast<const uint32_t*>(sb - sh);
	uint32_t* da = reinterpret_cast<uint32_t*>(dp + head);
	if (sh == 0) {
		for (int j = lane; j < nd; j += 64) da[j] = sa[j];
	} else {
		const unsigned r = 8u * sh, l = 32u - r;
		for (int j = lane; j < nd; j += 64) da[j] = (sa[j] >> r) | (sa[j + 1] << l);
	}
	if (lane < tail) dp[head + 4 * nd + lane] = sp[head + 4 * nd + lane];
}

// ------------------------------------------------------------------------------------------------ host side
struct State {
	Event ev_last;                            // behind the last call's kernels: the next call, on whatever stream, starts after it (they share the scratch below)
	bool used = false;
	DevBuf<Ctl> d_ctl;
	DevBuf<unsigned long long> d_table;       // the remembered headers: open addressing, full 48-bit keys | KEY_TAG, never more than half full
	int cap_log2 = 0;                         // 0: no table yet
	DevBuf<uint8_t> d_scratch;                // the call's table, kept words, bases, count
	DevBuf<uint8_t> d_in;                     // staging for host-memory input
	DevBuf<uint8_t> d_out;                    // ... and output
};

// what the entry points need of a context (filled by the context's mode: host.hip.inc delivery_view)
struct View {
	int device = 0;
	std::string* err = nullptr;
	hipStream_t stream = nullptr;
	int chunk = 0, per = 0;
	std::unique_ptr<State>* state = nullptr;
};

#define DELIVER_CHK(call)                                                                                \
	do {                                                                                                  \
		hipError_t e__ = (call);                                                                          \
		if (e__ != hipSuccess) {                                                                          \
			*v.err = std::string(#call) + ": " + hipGetErrorString(e__);                                  \
			return CIMBAR_HIP_EHIP;                                                                       \
		}                                                                                                 \
	} while (0)

int ensure_state(const View& v)
{
	if (*v.state) return 0;
	std::unique_ptr<State> s(new State);
	DELIVER_CHK(s->ev_last.create());
	DELIVER_CHK(s->d_ctl.reserve(1));
	DELIVER_CHK(hipMemset(s->d_ctl, 0, sizeof(Ctl)));
	*v.state = std::move(s);
	return 0;
}

// everything the last call enqueued is over (before a buffer it may still use is freed, or its results are read)
int quiesce(const View& v, State* s)
{
	if (s->used) DELIVER_CHK(hipEventSynchronize(s->ev_last));
	return 0;
}

// room for `need` bytes in one of the state's buffers, replaced only once nothing in flight uses it
int reserve_idle(const View& v, State* s, DevBuf<uint8_t>& buf, size_t need)
{
	if (need <= buf.capacity()) return 0;
	if (int r = quiesce(v, s)) return r;
	DELIVER_CHK(buf.reserve(need));
	return 0;
}

// (re)creates the persistent table with 2^cap_log2 free entries and clears the counters
int reset_table(const View& v, State* s, int cap_log2)
{
	if (int r = quiesce(v, s)) return r;
	if (s->cap_log2 != cap_log2) {
		s->cap_log2 = 0;
		DELIVER_CHK(s->d_table.release());   // (a smaller table is a smaller allocation)
		DELIVER_CHK(s->d_table.reserve((size_t)1 << cap_log2));
		s->cap_log2 = cap_log2;
	}
	DELIVER_CHK(hipMemset(s->d_table, 0, sizeof(unsigned long long) << cap_log2));
	DELIVER_CHK(hipMemset(s->d_ctl, 0, sizeof(Ctl)));
	DELIVER_CHK(hipDeviceSynchronize());
	return 0;
}

inline size_t up8(size_t x) { return (x + 7u) & ~(size_t)7u; }

int64_t deliver_chunks(const View& v, const uint8_t* chunks, const uint32_t* masks, int n, int in_mem, unsigned flags, uint8_t* packed, int32_t* src,
                       int32_t* count, int out_mem, void* hip_stream)
{
	// arguments first: nothing below this block runs for a call that is refused
	if (!chunks || !masks || !packed || !count || n <= 0) { *v.err = "deliver_chunks: null buffer or n <= 0"; return CIMBAR_HIP_EINVAL; }
	if (flags & ~ALL_FLAGS) { *v.err = "deliver_chunks: unknown flag bits"; return CIMBAR_HIP_EINVAL; }
	if ((in_mem != CIMBAR_HIP_MEM_HOST && in_mem != CIMBAR_HIP_MEM_DEVICE) || (out_mem != CIMBAR_HIP_MEM_HOST && out_mem != CIMBAR_HIP_MEM_DEVICE)) {
		*v.err = "deliver_chunks: in_mem / out_mem must be CIMBAR_HIP_MEM_HOST or CIMBAR_HIP_MEM_DEVICE";
		return CIMBAR_HIP_EINVAL;
	}
	if ((long long)n * v.per > MAX_SLOTS) { *v.err = "deliver_chunks: more than 2^24 slots in one call"; return CIMBAR_HIP_EINVAL; }
	if (flags & CIMBAR_HIP_DELIVER_REMEMBER) flags |= CIMBAR_HIP_DELIVER_DEDUP;
	const bool dedup = flags & CIMBAR_HIP_DELIVER_DEDUP, remember = flags & CIMBAR_HIP_DELIVER_REMEMBER;

	DELIVER_CHK(hipSetDevice(v.device));
	if (int r = ensure_state(v)) return r;
	State* s = v.state->get();
	// the stream rules of cimbar_hip_decode_batch: NULL is the null stream when a device buffer is involved, the context's own stream otherwise
	// (host.hip.inc's begin_call restated, not called: this code is shared by every mode and sees a context through a View only; it touches no
	// scratch set, so it waits for no pipelined batch)
	const bool any_device = in_mem == CIMBAR_HIP_MEM_DEVICE || out_mem == CIMBAR_HIP_MEM_DEVICE;
	hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (any_device ? (hipStream_t)nullptr : v.stream);

	const int total = n * v.per, cs = v.chunk;
	uint32_t tsize = 0;   // the call's table: a power of two, at least twice the candidates
	if (dedup) for (tsize = 16; tsize < 2u * (uint32_t)total; tsize <<= 1) {}
	const size_t off_kept = up8(sizeof(unsigned long long) * tsize), off_first = up8(off_kept + sizeof(uint32_t) * (size_t)n),
	             off_where = up8(off_first + sizeof(uint32_t) * tsize), off_base = up8(off_where + sizeof(int32_t) * (size_t)total),
	             off_count = up8(off_base + sizeof(uint32_t) * (size_t)n), need = off_count + 8;
	if (int r = reserve_idle(v, s, s->d_scratch, need)) return r;
	const size_t in_bytes = up8((size_t)total * cs), out_bytes = up8((size_t)total * cs);
	if (in_mem == CIMBAR_HIP_MEM_HOST) if (int r = reserve_idle(v, s, s->d_in, in_bytes + sizeof(uint32_t) * (size_t)n)) return r;
	if (out_mem == CIMBAR_HIP_MEM_HOST) if (int r = reserve_idle(v, s, s->d_out, out_bytes + sizeof(int32_t) * (size_t)total)) return r;
	if (remember && !s->cap_log2) if (int r = reset_table(v, s, DEFAULT_CAP_LOG2)) return r;

	if (s->used) DELIVER_CHK(hipStreamWaitEvent(st, s->ev_last, 0));
	const uint8_t* d_chunks = chunks;
	const uint32_t* d_masks = masks;
	if (in_mem == CIMBAR_HIP_MEM_HOST) {
		DELIVER_CHK(hipMemcpyAsync(s->d_in, chunks, (size_t)total * cs, hipMemcpyHostToDevice, st));
		DELIVER_CHK(hipMemcpyAsync(s->d_in + in_bytes, masks, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
		d_chunks = s->d_in;
		d_masks = reinterpret_cast<const uint32_t*>(s->d_in + in_bytes);
	}
	uint8_t* d_packed = out_mem == CIMBAR_HIP_MEM_DEVICE ? packed : s->d_out.get();
	int32_t* d_src = out_mem == CIMBAR_HIP_MEM_DEVICE ? src : (src ? reinterpret_cast<int32_t*>(s->d_out + out_bytes) : nullptr);
	unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(s->d_scratch.get());
	uint32_t* d_kept = reinterpret_cast<uint32_t*>(s->d_scratch + off_kept);
	uint32_t* d_first = reinterpret_cast<uint32_t*>(s->d_scratch + off_first);
	int32_t* d_where = reinterpret_cast<int32_t*>(s->d_scratch + off_where);
	uint32_t* d_base = reinterpret_cast<uint32_t*>(s->d_scratch + off_base);
	int32_t* d_count = out_mem == CIMBAR_HIP_MEM_DEVICE ? count : reinterpret_cast<int32_t*>(s->d_scratch + off_count);
	const uint32_t capacity = remember ? 1u << s->cap_log2 : 0u;

	DELIVER_CHK(hipMemsetAsync(s->d_scratch, 0, off_first, st));                                   // free keys, kept = 0
	if (dedup) DELIVER_CHK(hipMemsetAsync(d_first, 0xFF, sizeof(uint32_t) * (size_t)tsize, st));   // no candidate yet
	const unsigned lanes_grid = (unsigned)((total + 255) / 256), waves_grid = (unsigned)((total + 3) / 4);
	hipLaunchKernelGGL(k_deliver_mark, dim3(lanes_grid), dim3(256), 0, st, d_chunks, d_masks, total, v.per, cs, flags, d_keys, d_first, tsize - 1u, d_where);
	hipLaunchKernelGGL(k_deliver_select, dim3(lanes_grid), dim3(256), 0, st, d_where, total, v.per, flags, d_keys, d_first, s->d_table, capacity - 1u, d_kept);
	hipLaunchKernelGGL(k_deliver_scan, dim3(1), dim3(1024), 0, st, d_kept, n, d_base, d_count, flags, s->d_ctl, capacity);
	hipLaunchKernelGGL(k_deliver_copy, dim3(waves_grid), dim3(256), 0, st, d_chunks, d_kept, d_base, total, v.per, cs, d_packed, d_src, flags, d_where, d_keys,
	                   s->d_ctl, s->d_table, capacity - 1u);
	DELIVER_CHK(hipGetLastError());
	DELIVER_CHK(hipEventRecord(s->ev_last, st));
	s->used = true;
	if (out_mem == CIMBAR_HIP_MEM_DEVICE) return 0;

	int32_t got = 0;
	DELIVER_CHK(hipMemcpyAsync(&got, d_count, sizeof got, hipMemcpyDeviceToHost, st));
	DELIVER_CHK(hipStreamSynchronize(st));
	if (got > 0) {   // only what was delivered crosses, and only that much of the caller's buffers is written
		DELIVER_CHK(hipMemcpyAsync(packed, d_packed, (size_t)got * cs, hipMemcpyDeviceToHost, st));
		if (src) DELIVER_CHK(hipMemcpyAsync(src, d_src, sizeof(int32_t) * (size_t)got, hipMemcpyDeviceToHost, st));
		DELIVER_CHK(hipStreamSynchronize(st));
	}
	*count = got;
	return got;
}

int delivery_reset(const View& v, int capacity_log2)
{
	if (capacity_log2 != 0 && (capacity_log2 < MIN_CAP_LOG2 || capacity_log2 > MAX_CAP_LOG2)) {
		*v.err = "delivery_reset: capacity_log2 must be 0 (the default, 20) or 4 .. 24";
		return CIMBAR_HIP_EINVAL;
	}
	DELIVER_CHK(hipSetDevice(v.device));
	if (int r = ensure_state(v)) return r;
	return reset_table(v, v.state->get(), capacity_log2 ? capacity_log2 : DEFAULT_CAP_LOG2);
}

int delivery_stats(const View& v, int64_t* remembered, int64_t* capacity, int* overflowed)
{
	Ctl c{};
	State* s = v.state->get();
	if (s) {
		DELIVER_CHK(hipSetDevice(v.device));
		if (int r = quiesce(v, s)) return r;
		DELIVER_CHK(hipMemcpy(&c, s->d_ctl, sizeof c, hipMemcpyDeviceToHost));
	}
	if (remembered) *remembered = c.remembered;
	if (capacity) *capacity = s && s->cap_log2 ? (int64_t)1 << s->cap_log2 : 0;
	if (overflowed) *overflowed = c.overflowed ? 1 : 0;
	return 0;
}

#undef DELIVER_CHK

}  // namespace

}  // namespace deliver
