// pair_io.h -- buffer addressing and hand-counted prefetch of the persistent float-frame kernels (pair.hip, quad.hip, wide.hip).
#pragma once
#include "kernels.h"

namespace bfir {

namespace {

// Buffer addressing for the persistent kernels: a wave-uniform descriptor (4 SGPRs) + one 32-bit lane
// offset + a scalar offset per access, instead of a 64-bit address pair in VGPRs per access (the
// one-block-per-workgroup kernels spent a quarter of their vector instructions and ~20 registers on those).
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, unsigned bytes)
{
    // the pointer is workgroup-uniform by construction; readfirstlane tells the compiler so
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float2 buf_load2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    float2 f; f.x = __uint_as_float(v.x); f.y = __uint_as_float(v.y);
    return f;
}
template <int AUX = 0>   // cache policy bits of the instruction: 2 = nt
__device__ __forceinline__ void buf_store4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, float4 f)
{
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    u4 v; v.x = __float_as_uint(f.x); v.y = __float_as_uint(f.y); v.z = __float_as_uint(f.z); v.w = __float_as_uint(f.w);
    __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, soff, AUX);
}
__device__ __forceinline__ void buf_store2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, float2 f)
{
    u32x2 v; v.x = __float_as_uint(f.x); v.y = __float_as_uint(f.y);
    __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, 0);
}

// Prefetch loads the compiler must not wait for.  hipcc's s_waitcnt bookkeeping gives up at the head of
// the transform loop ("vmcnt(0)": wait for everything, i.e. also for the spectrum stores of the previous
// transform, which is exactly the overlap this kernel exists for).  So the in-loop prefetch is issued from
// an asm statement (invisible to that bookkeeping) and waited for by hand with a counted vmcnt: vector
// memory operations retire in issue order, so "all but the N youngest" with N = the stores issued after
// the prefetch is precisely "the prefetch has landed".  (cdna_hip_programming.md 5.7 form (ii): "+v"
// operands on load and wait statements pin the order; the .s is audited for copies in between.)
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_rsrc_words(const void *p, unsigned bytes)
{
    const unsigned long long u = (unsigned long long)p;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)u);
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));   // stride 0
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}
// 8 x 8 bytes per lane: d[e] <- buffer[voff + e * step]
__device__ __forceinline__ void asm_prefetch8x2(u32x2 (&d)[8], unsigned voff, i32x4 r, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1, s4 = 4 * s1, s5 = 5 * s1, s6 = 6 * s1, s7 = 7 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_load_dwordx2 %0, %8, %9, 0 offen\n\t"
                 "buffer_load_dwordx2 %1, %8, %9, %10 offen\n\t"
                 "buffer_load_dwordx2 %2, %8, %9, %11 offen\n\t"
                 "buffer_load_dwordx2 %3, %8, %9, %12 offen\n\t"
                 "buffer_load_dwordx2 %4, %8, %9, %13 offen\n\t"
                 "buffer_load_dwordx2 %5, %8, %9, %14 offen\n\t"
                 "buffer_load_dwordx2 %6, %8, %9, %15 offen\n\t"
                 "buffer_load_dwordx2 %7, %8, %9, %16 offen"
                 : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7])
                 : "v"(voff), "s"(r), "s"(s1), "s"(s2), "s"(s3), "s"(s4), "s"(s5), "s"(s6), "s"(s7)
                 : "memory");
}
// 8 x 16 bytes per lane: a[j] <- buffer A[voff + j * step], b[j] <- buffer B[...]   (j < 4)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void asm_prefetch2x4x4(u32x4 (&a)[4], u32x4 (&b)[4], unsigned voff, i32x4 ra, i32x4 rb, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_load_dwordx4 %0, %8, %9, 0 offen nt\n\t"
                 "buffer_load_dwordx4 %4, %8, %10, 0 offen nt\n\t"
                 "buffer_load_dwordx4 %1, %8, %9, %11 offen nt\n\t"
                 "buffer_load_dwordx4 %5, %8, %10, %11 offen nt\n\t"
                 "buffer_load_dwordx4 %2, %8, %9, %12 offen nt\n\t"
                 "buffer_load_dwordx4 %6, %8, %10, %12 offen nt\n\t"
                 "buffer_load_dwordx4 %3, %8, %9, %13 offen nt\n\t"
                 "buffer_load_dwordx4 %7, %8, %10, %13 offen nt"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 : "v"(voff), "s"(ra), "s"(rb), "s"(s1), "s"(s2), "s"(s3)
                 : "memory");
}
// 8 x 16 bytes per lane: buffer[voff + k * step] <- d[k].  One asm statement that ENDS in a wait state: left to the
// compiler (raw_buffer_store_b128 with a register offset) the instruction after a store was a VALU write of the store's
// first data register -- in k_inv_quad_ps the next piece's overflow count -- and on the GPU that value (0) went out in
// place of channel 4q's sample in some lanes of some launches.  Data registers of a 16-byte store must not be written in
// the slot behind it (cdna_hip_programming.md 5.7 item 1, stores); the opening s_nop covers the descriptor fresh from
// readfirstlane.  (quad.hip: the output frames; wide.hip: the history frames.)
__device__ __forceinline__ void asm_store8x4(const u32x4 (&d)[8], unsigned voff, i32x4 r, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1, s4 = 4 * s1, s5 = 5 * s1, s6 = 6 * s1, s7 = 7 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_store_dwordx4 %0, %8, %9, 0 offen\n\t"
                 "buffer_store_dwordx4 %1, %8, %9, %10 offen\n\t"
                 "buffer_store_dwordx4 %2, %8, %9, %11 offen\n\t"
                 "buffer_store_dwordx4 %3, %8, %9, %12 offen\n\t"
                 "buffer_store_dwordx4 %4, %8, %9, %13 offen\n\t"
                 "buffer_store_dwordx4 %5, %8, %9, %14 offen\n\t"
                 "buffer_store_dwordx4 %6, %8, %9, %15 offen\n\t"
                 "buffer_store_dwordx4 %7, %8, %9, %16 offen\n\t"
                 "s_nop 1"
                 :
                 : "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]), "v"(d[4]), "v"(d[5]), "v"(d[6]), "v"(d[7]),
                   "v"(voff), "s"(r), "s"(s1), "s"(s2), "s"(s3), "s"(s4), "s"(s5), "s"(s6), "s"(s7)
                 : "memory");
}
// 2 x 8 x 4 bytes per lane (time pairs: one channel's samples of two blocks): b[e] <- buffer B[voff + e * step], c[e] <- buffer C[...]
__device__ __forceinline__ void asm_prefetch2x8x1(unsigned (&b)[8], unsigned (&c)[8], unsigned voff, i32x4 rb, i32x4 rc, unsigned step)
{
    const unsigned s1 = __builtin_amdgcn_readfirstlane(step), s2 = 2 * s1, s3 = 3 * s1, s4 = 4 * s1, s5 = 5 * s1, s6 = 6 * s1, s7 = 7 * s1;
    asm volatile("s_nop 4\n\t"
                 "buffer_load_dword %0, %16, %17, 0 offen\n\t"
                 "buffer_load_dword %8, %16, %18, 0 offen\n\t"
                 "buffer_load_dword %1, %16, %17, %19 offen\n\t"
                 "buffer_load_dword %9, %16, %18, %19 offen\n\t"
                 "buffer_load_dword %2, %16, %17, %20 offen\n\t"
                 "buffer_load_dword %10, %16, %18, %20 offen\n\t"
                 "buffer_load_dword %3, %16, %17, %21 offen\n\t"
                 "buffer_load_dword %11, %16, %18, %21 offen\n\t"
                 "buffer_load_dword %4, %16, %17, %22 offen\n\t"
                 "buffer_load_dword %12, %16, %18, %22 offen\n\t"
                 "buffer_load_dword %5, %16, %17, %23 offen\n\t"
                 "buffer_load_dword %13, %16, %18, %23 offen\n\t"
                 "buffer_load_dword %6, %16, %17, %24 offen\n\t"
                 "buffer_load_dword %14, %16, %18, %24 offen\n\t"
                 "buffer_load_dword %7, %16, %17, %25 offen\n\t"
                 "buffer_load_dword %15, %16, %18, %25 offen"
                 : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7])
                 : "v"(voff), "s"(rb), "s"(rc), "s"(s1), "s"(s2), "s"(s3), "s"(s4), "s"(s5), "s"(s6), "s"(s7)
                 : "memory");
}
template <int N> __device__ __forceinline__ void asm_wait_vmcnt(unsigned (&b)[8], unsigned (&c)[8])
{
    asm volatile("s_waitcnt vmcnt(%16)"
                 : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]),
                   "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7])
                 : "n"(N) : "memory");
}
// wait until all but the N youngest vector-memory operations of this wave are done; names the prefetch
// destinations so that no use of them is scheduled above it
template <int N, typename V, int K> __device__ __forceinline__ void asm_wait_vmcnt(V (&d)[K])
{
    static_assert(K == 8, "eight destinations");
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(d[0]), "+v"(d[1]), "+v"(d[2]), "+v"(d[3]), "+v"(d[4]), "+v"(d[5]), "+v"(d[6]), "+v"(d[7])
                 : "n"(N) : "memory");
}
template <int N, typename V> __device__ __forceinline__ void asm_wait_vmcnt(V (&a)[4], V (&b)[4])
{
    asm volatile("s_waitcnt vmcnt(%8)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3])
                 : "n"(N) : "memory");
}

__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    float4 f; f.x = __uint_as_float(v.x); f.y = __uint_as_float(v.y); f.z = __uint_as_float(v.z); f.w = __uint_as_float(v.w);
    return f;
}

// Minimum waves per SIMD the inverse kernel is compiled for.  Four (128 registers) everywhere but N = 4096, whose
// last pass is a radix-16 one with six base twiddles in registers: at 128 it spills ONE register, and a spill is a
// scratch (vector-memory) operation inside the window the hand-counted vmcnt spans -- the wait would then cover
// one operation too few.  scripts/audit_ps_isa.py (tests/test_isa_audit.py) found it and checks every build.
template <int LOG2N> constexpr int inv_ps_min_waves() { return LOG2N == 12 ? 3 : 4; }

}  // namespace

}  // namespace bfir
