// Fragment of egotap_abi.hip, included there exactly once; it includes nothing.  The order of the fragments there fixes hipcc's schedules.
// The zero-fill kernel and its launcher.
// stream-ordered zero fill as a KERNEL: a hipMemsetAsync captured into a HIP graph did not re-execute on replay (ROCm 7.2: the
// propagation units' cell state then carried over from one replay to the next), a kernel node does
static __global__ __launch_bounds__(256) void zero_fill_kernel(f32x4* __restrict__ p, long n16) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}
static hipError_t zero_fill(void* p, size_t bytes, hipStream_t s) {       // p 16-byte aligned, bytes a multiple of 16
    if (bytes == 0) return hipSuccess;
    if ((((uintptr_t)p) | bytes) & 15) return hipErrorInvalidValue;
    const long n16 = (long)(bytes / 16);
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, (f32x4*)p, n16);
    return hipGetLastError();
}
