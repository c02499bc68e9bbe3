// wt_store.h -- write-through (sc1) stores for the buffers one kernel of the training step hands to the
// next. Each XCD has a private write-back L2: lines a kernel leaves dirty there are written back at its
// end, before the dependent kernel may start. An sc1 store sends the bytes on at once and keeps no line in
// the writer's L2, so the write-back overlaps the rest of the kernel instead of sitting on the boundary.
// Nothing else changes: no fence, wait or flag -- the kernel boundary orders the stores as before. A
// buffer written this way must not be read back by the same launch (the line is gone from this L2).
// The sites and their switch bits: EngineSwitches::wt_stores (runtime.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tcnn_amd {

// One bit per store site (TCNN_WT_STORES). Both end-of-kernel bursts; the sites that measured slower or
// within noise (dL/d(encoding), 4-byte stores spread over the fused kernel; k_adam's state) stay plain
// ("Store policy at the kernel boundaries").
enum : uint32_t {
	WT_WGRAD_SLAB = 1u,  // fused kernel: the workgroup's network-gradient slab (epilogue)
	WT_GRID_SLAB = 2u,   // grid backward: the chunk slab of every workgroup
	WT_STORES_ALL = 3u,
	WT_STORES_DEFAULT = WT_STORES_ALL,
};

// 4- or 8-byte value -> global_store_dword / dwordx2 ... sc1
template <typename T>
__device__ __forceinline__ void wt_store(T* p, T v) {
	static_assert(sizeof(T) == 4 || sizeof(T) == 8, "wt_store: 4- or 8-byte values (16 bytes: wt_store16)");
	if constexpr (sizeof(T) == 4)
		__hip_atomic_store((uint32_t*)p, __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	else
		__hip_atomic_store((unsigned long long*)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16-byte stores go through a buffer resource (buffer_store_dwordx4 ... sc1). Build it once per workgroup
// at the workgroup's own destination base (wave-uniform), so byte offsets and the record count stay small
// whatever the whole buffer's size; stores past `bytes` are dropped by the range check.
typedef __amdgpu_buffer_rsrc_t wt_rsrc;
__device__ __forceinline__ wt_rsrc wt_make_rsrc(void* base, uint32_t bytes) {
	return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
}
template <typename T>
__device__ __forceinline__ void wt_store16(wt_rsrc r, uint32_t byte_offset, T v) {
	static_assert(sizeof(T) == 16, "wt_store16: 16-byte values");
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	__builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_offset, 0, 16);  // aux 16 = sc1
}

}  // namespace tcnn_amd
