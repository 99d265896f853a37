// Internal (not part of the C-ABI): the 32-rows-per-wave attention kernels of attn32.hip, planned and launched by attn.hip (attn_plan_fwd / _bwd, attn_launch).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/sdlt_kernels.h"
bool sdlt_attn32_ok(const sdlt_attn_params& p);
// the kernel of `ks` wave groups (1, 2 or 4; 128 * ks threads) and its dynamic LDS bytes
struct sdlt_attn32_kernel { void (*fn)(const sdlt_attn_params); int smem; };
sdlt_attn32_kernel sdlt_attn32_fwd(int ks);
sdlt_attn32_kernel sdlt_attn32_bwd_both(int ks);
