// Probe for K1's colour column sums (not part of the product): what does v_mqsad_pk_u16_u8 cost to issue on gfx950 next to v_add_u32, and does it
// compute what the column sums need? With the reference operand 0x000000FF only byte 0 of the reference is non-zero, so of each of the four byte
// windows of the 64-bit source (starting at its bytes 0..3) only the first byte counts: one instruction adds 255 - byte j of a dword to the j-th of
// four u16 accumulators.
//   hipcc --offload-arch=gfx950 -O3 -o mqsad_probe tools/mqsad_probe.hip && ./mqsad_probe
// Part 1 checks the instruction against a host loop on random dwords (reference 0xFF, and 0xFF00 / 0xFF000000 to see where the windows start; the
// source's high dword is random too: with 0xFF it must not matter). Part 2 times chains of independent instructions, 8 accumulators per lane,
// 8 wavefronts per SIMD on every CU, a few seconds in all.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__global__ void k_check(const uint64_t* __restrict__ src, const uint64_t* __restrict__ acc, uint32_t ref, uint64_t* __restrict__ out, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = __builtin_amdgcn_mqsad_pk_u16_u8(src[i], ref, acc[i]);
}

static uint64_t host_mqsad(uint64_t s, uint32_t ref, uint64_t acc)
{
	uint64_t r = 0;
	for (int i = 0; i < 4; ++i) {
		uint32_t sum = (uint32_t)((acc >> (16 * i)) & 0xFFFF);
		for (int k = 0; k < 4; ++k) {
			const int rb = (ref >> (8 * k)) & 0xFF, sb = (int)((s >> (8 * (i + k))) & 0xFF);
			if (rb) sum += (uint32_t)(sb > rb ? sb - rb : rb - sb);   // bytes of the reference that are 0 are skipped
		}
		r |= (uint64_t)(sum & 0xFFFF) << (16 * i);
	}
	return r;
}

// OP 0: v_add_u32, OP 1: v_mqsad_pk_u16_u8 with the reference in a VGPR, OP 2: with the reference in an SGPR, OP 3: v_mov_b64 (what the compiler
// adds where an accumulator pair has to come back to its register). 8 independent chains per lane; the SAD
// chains alternate between two register pairs because the instruction's destination may not overlap its sources.
template <int OP>
__global__ __launch_bounds__(256) void k_rate(uint32_t* __restrict__ out, int iters, uint32_t seed)
{
	uint32_t x = seed + threadIdx.x, r = 0xFFu;
	uint64_t xs = ((uint64_t)(x * 2654435761u) << 32) | x;
	uint32_t a[8];
	uint64_t p[8], q[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) { a[k] = k; p[k] = k; q[k] = 0; }
	for (int it = 0; it < iters; ++it) {
#pragma unroll
		for (int u = 0; u < 4; ++u) {
#pragma unroll
			for (int k = 0; k < 8; ++k) {
				if (OP == 0) {
					asm volatile("v_add_u32 %0, %1, %0" : "+v"(a[k]) : "v"(x));
					asm volatile("v_add_u32 %0, %1, %0" : "+v"(a[k]) : "v"(x));
				} else if (OP == 1) {
					asm volatile("v_mqsad_pk_u16_u8 %0, %1, %2, %3" : "=&v"(q[k]) : "v"(xs), "v"(r), "v"(p[k]));
					asm volatile("v_mqsad_pk_u16_u8 %0, %1, %2, %3" : "=&v"(p[k]) : "v"(xs), "v"(r), "v"(q[k]));
				} else if (OP == 2) {
					asm volatile("v_mqsad_pk_u16_u8 %0, %1, %2, %3" : "=&v"(q[k]) : "v"(xs), "s"(0xFFu), "v"(p[k]));
					asm volatile("v_mqsad_pk_u16_u8 %0, %1, %2, %3" : "=&v"(p[k]) : "v"(xs), "s"(0xFFu), "v"(q[k]));
				} else {
					asm volatile("v_mov_b64 %0, %1" : "=v"(q[k]) : "v"(p[k]));
					asm volatile("v_mov_b64 %0, %1" : "=v"(p[k]) : "v"(q[k]));
				}
			}
		}
	}
	uint32_t s = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) s ^= a[k] ^ (uint32_t)p[k] ^ (uint32_t)(p[k] >> 32);
	if (s == 0x12345678u) out[0] = s;
}

template <int OP> static int rate(const char* label, uint32_t* d_out, int blocks, double* ms_out)
{
	const int iters = 1 << 16, launches = 8;   // 64 instructions per iteration and chain set
	hipEvent_t a, b;
	CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
	hipLaunchKernelGGL(k_rate<OP>, dim3(blocks), dim3(256), 0, 0, d_out, iters, 1u);
	CK(hipDeviceSynchronize());
	CK(hipEventRecord(a));
	for (int l = 0; l < launches; ++l) hipLaunchKernelGGL(k_rate<OP>, dim3(blocks), dim3(256), 0, 0, d_out, iters, (uint32_t)l);
	CK(hipEventRecord(b));
	CK(hipEventSynchronize(b));
	float ms;
	CK(hipEventElapsedTime(&ms, a, b));
	const double per_wave = (double)launches * iters * 64;
	printf("%-44s %9.1f ms   %.3f ns per wavefront instruction per SIMD\n", label, ms, ms * 1e6 / (per_wave * 8));
	*ms_out = ms;
	return 0;
}

int main()
{
	const int n = 1 << 20;
	std::mt19937_64 g(12345);
	std::vector<uint64_t> src(n), acc(n), got(n);
	for (int i = 0; i < n; ++i) {
		src[i] = g();
		const uint64_t v = g();
		acc[i] = v & 0x1FFF1FFF1FFF1FFFull;   // (below 8192 per u16: no sum of this check wraps)
	}
	for (int i = 0; i < 256; ++i) src[i] = (src[i] & ~0xFFFFFFFFull) | (i < 128 ? 0u : 0xFFFFFFFFu);   // both ends of the column sums too
	uint64_t *d_src, *d_acc, *d_out;
	CK(hipMalloc(&d_src, n * 8)); CK(hipMalloc(&d_acc, n * 8)); CK(hipMalloc(&d_out, n * 8));
	CK(hipMemcpy(d_src, src.data(), n * 8, hipMemcpyHostToDevice));
	CK(hipMemcpy(d_acc, acc.data(), n * 8, hipMemcpyHostToDevice));
	int bad_total = 0;
	for (uint32_t ref : {0x000000FFu, 0x0000FF00u, 0xFF000000u, 0x00FF00FFu}) {
		hipLaunchKernelGGL(k_check, dim3(n / 256), dim3(256), 0, 0, d_src, d_acc, ref, d_out, n);
		CK(hipMemcpy(got.data(), d_out, n * 8, hipMemcpyDeviceToHost));
		int bad = 0, low_only = 0;
		for (int i = 0; i < n; ++i) {
			bad += got[i] != host_mqsad(src[i], ref, acc[i]);
			low_only += got[i] == host_mqsad(src[i] & 0xFFFFFFFFull, ref, acc[i]);
		}
		printf("reference %08x: %d of %d results differ from the host loop (%d equal the host loop on the low dword alone)\n", ref, bad, n, low_only);
		bad_total += bad;
	}
	hipDeviceProp_t prop;
	CK(hipGetDeviceProperties(&prop, 0));
	const int blocks = prop.multiProcessorCount * 8;   // 8 workgroups of 4 wavefronts per CU: 8 wavefronts per SIMD
	printf("%d CUs, %d workgroups of 256\n", prop.multiProcessorCount, blocks);
	double add = 0, sadv = 0, sads = 0, mov64 = 0, add2 = 0;
	if (rate<0>("v_add_u32", (uint32_t*)d_out, blocks, &add)) return 1;
	if (rate<1>("v_mqsad_pk_u16_u8, reference in a VGPR", (uint32_t*)d_out, blocks, &sadv)) return 1;
	if (rate<2>("v_mqsad_pk_u16_u8, reference in an SGPR", (uint32_t*)d_out, blocks, &sads)) return 1;
	if (rate<3>("v_mov_b64", (uint32_t*)d_out, blocks, &mov64)) return 1;
	if (rate<0>("v_add_u32 again", (uint32_t*)d_out, blocks, &add2)) return 1;
	printf("issue cost in v_add_u32: v_mqsad_pk_u16_u8 %.2f (VGPR reference), %.2f (SGPR reference), v_mov_b64 %.2f; the two v_add_u32 runs differ by %.1f %%\n",
	       sadv / add, sads / add, mov64 / add, 100.0 * (add2 - add) / add);
	return bad_total ? 2 : 0;
}
