// stream_sum.hip -- the yardstick of tools/dbscan_bench.py: a plain streaming
// read of a device buffer, 16 bytes a lane, summed so that no load can be
// dropped.  Built by the tool into tools/micro/libstream_sum.so:
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libstream_sum.so stream_sum.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void k_stream_sum(const uint4 *__restrict__ p, long long nvec,
                                                    unsigned long long *__restrict__ out) {
	unsigned long long s = 0;
	const long long stride = (long long) gridDim.x * blockDim.x;
	long long v = (long long) blockIdx.x * blockDim.x + threadIdx.x;
	for(; v + 3 * stride < nvec; v += 4 * stride) {   // four loads in flight per lane
		const uint4 a = p[v], b = p[v + stride], c = p[v + 2 * stride], d = p[v + 3 * stride];
		s += (unsigned long long) a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
		s += (unsigned long long) c.x + c.y + c.z + c.w + d.x + d.y + d.z + d.w;
	}
	for(; v < nvec; v += stride) {
		const uint4 a = p[v];
		s += (unsigned long long) a.x + a.y + a.z + a.w;
	}
	for(int o = 32; o; o >>= 1) s += __shfl_down(s, o);
	if((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

extern "C" {
// enqueues one pass over `bytes` (a multiple of 16) on the null stream; *out_dev accumulates the sum
int stream_sum(const void *p, size_t bytes, unsigned long long *out_dev, int blocks) {
	k_stream_sum<<<blocks, 256>>>((const uint4 *) p, (long long) (bytes / 16), out_dev);
	return (int) hipGetLastError();
}
int stream_sync(void) { return (int) hipDeviceSynchronize(); }
}
