// f64_rate.hip -- the yardstick of tools/vec_bench.py: the issue rate of plain
// v_mul_f64 + v_add_f64 pairs (no FMA: the vec kernel's cos step, d += x * y
// with product and sum rounded apart), 16 independent chains per lane from
// registers, no memory traffic in the loop.  Built by the tool into
// tools/micro/libf64_rate.so:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC -o libf64_rate.so f64_rate.hip
#include <hip/hip_runtime.h>

__global__ __launch_bounds__(256) void k_f64_rate(const double *__restrict__ in, double *__restrict__ out, int iters) {
	double x[4], y[4], d[4][4];
	for(int a = 0; a < 4; ++a) {
		x[a] = in[threadIdx.x * 8 + a];
		y[a] = in[threadIdx.x * 8 + 4 + a];
		for(int b = 0; b < 4; ++b) d[a][b] = 0;
	}
	for(int it = 0; it < iters; ++it) {
#pragma unroll
		for(int a = 0; a < 4; ++a) {
			asm volatile("" : "+v"(x[a]), "+v"(y[a]));   // keeps the products inside the loop
#pragma unroll
			for(int b = 0; b < 4; ++b) d[a][b] += x[a] * y[b];
		}
	}
	double s = 0;
	for(int a = 0; a < 4; ++a)
		for(int b = 0; b < 4; ++b) s += d[a][b];
	if(s == 12345.678) out[0] = s;   // never true for the tool's input; keeps the chains alive
}

extern "C" {
// runs `blocks` blocks of 256 lanes for `iters` iterations of 16 mul + add pairs a lane on the null stream and
// returns the pairs per second over all lanes (0 on a HIP error); `in`: 2048 doubles, `out`: one
double f64_pair_rate(const double *in, double *out, int blocks, int iters) {
	hipEvent_t e0, e1;
	if(hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 0;
	k_f64_rate<<<blocks, 256>>>(in, out, iters / 8 + 1);   // warm-up
	(void) hipEventRecord(e0, 0);
	k_f64_rate<<<blocks, 256>>>(in, out, iters);
	(void) hipEventRecord(e1, 0);
	float ms = 0;
	const bool ok = hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
	                hipGetLastError() == hipSuccess && ms > 0;
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	return ok ? (double) blocks * 256.0 * (double) iters * 16.0 / (ms * 1e-3) : 0;
}
}
