// stream_rw.hip -- the yardstick of tools/merge_bench.py: a plain streaming
// read-and-write of a device buffer in place, 16 bytes a lane, every word
// changed so that neither the load nor the store can be dropped.  Built by the
// tool into tools/micro/libstream_rw.so:
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libstream_rw.so stream_rw.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void k_stream_rw(uint4 *__restrict__ p, long long nvec) {
	const long long stride = (long long) gridDim.x * blockDim.x;
	long long v = (long long) blockIdx.x * blockDim.x + threadIdx.x;
	for(; v + 3 * stride < nvec; v += 4 * stride) {   // four loads in flight per lane
		uint4 a = p[v], b = p[v + stride], c = p[v + 2 * stride], d = p[v + 3 * stride];
		a.x ^= 1u; a.y ^= 1u; a.z ^= 1u; a.w ^= 1u;
		b.x ^= 1u; b.y ^= 1u; b.z ^= 1u; b.w ^= 1u;
		c.x ^= 1u; c.y ^= 1u; c.z ^= 1u; c.w ^= 1u;
		d.x ^= 1u; d.y ^= 1u; d.z ^= 1u; d.w ^= 1u;
		p[v] = a;
		p[v + stride] = b;
		p[v + 2 * stride] = c;
		p[v + 3 * stride] = d;
	}
	for(; v < nvec; v += stride) {
		uint4 a = p[v];
		a.x ^= 1u; a.y ^= 1u; a.z ^= 1u; a.w ^= 1u;
		p[v] = a;
	}
}

extern "C" {
// enqueues one pass over `bytes` (a multiple of 16) on the null stream: bytes read and bytes written
int stream_rw(void *p, size_t bytes, int blocks) {
	k_stream_rw<<<blocks, 256>>>((uint4 *) p, (long long) (bytes / 16));
	return (int) hipGetLastError();
}
int stream_sync(void) { return (int) hipDeviceSynchronize(); }
}
