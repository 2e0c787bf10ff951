/* In-kernel phase stamps of the K-sliced conv launches -- tools only, reached through include/nerfrpn_tools.h, NOT part of the drop-in
 * boundary (include/nerfrpn.h).
 *
 * nrpn_conv3d_fwd_stamped runs the launches nrpn_conv3d_fwd_ex would run for the same arguments -- the same plan, the same grid, the same
 * outputs and workspace partials bit for bit -- on diagnostic instantiations of the kernels in which wave 0 of every workgroup reads the
 * two device clocks at the phase boundaries below and one lane writes ONE record of NRPN_STAMP_WORDS 64-bit words into the caller's
 * buffer.  Record r of the conv launch is workgroup r; the records of the split-K epilogue launch follow the conv launch's.
 *
 * A stamp is a pair: the constant-rate device clock (s_memrealtime, 100 MHz: 10 ns per tick) and the shader-cycle clock (s_memtime).
 * Cycles are meaningful inside one record only.  Read the SHARES of a stamped launch, not its length: the stamps' fences forbid overlaps
 * the product kernels have. */
#ifndef NERFRPN_STAMPS_H
#define NERFRPN_STAMPS_H
#include "nerfrpn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NRPN_STAMP_VERSION 0x4E52535400000001ull /* word 0 of every record: 'NRST', format 1 */
#define NRPN_STAMP_WORDS 32                      /* uint64 words per record */
#define NRPN_STAMP_REALTIME_NS 10                /* ns per tick of the constant-rate clock */
#define NRPN_STAMP_MAX_SLICES 64

/* word 1: which kernel wrote the record */
#define NRPN_STAMP_KERNEL_CONV128 1  /* conv_igemm_kernel, 128-row tile */
#define NRPN_STAMP_KERNEL_CONV256 2  /* conv_igemm_big_kernel, 256x256 tile */
#define NRPN_STAMP_KERNEL_EPILOGUE 3 /* splitk_epilogue_kernel */

/* word order of a record (words a kernel has no value for are written as 0) */
#define NRPN_SW_VERSION 0
#define NRPN_SW_KERNEL 1
#define NRPN_SW_WG 2      /* workgroup index of its launch */
#define NRPN_SW_MTILE 3   /* conv: M tile */
#define NRPN_SW_NTILE 4   /* conv: N tile */
#define NRPN_SW_KSLICE 5  /* conv: K slice */
#define NRPN_SW_XCD 6     /* HW_REG_XCC_ID, 0..7 */
#define NRPN_SW_KSTEPS 7  /* conv: K-steps executed; epilogue: grid-stride iterations of lane 0 */
#define NRPN_SW_PHASE0 8  /* phase p: constant-rate clock at 8 + 2 p, shader cycles at 9 + 2 p */
#define NRPN_SW_WAIT_SUM 22 /* conv: cycles in the per-K-step wait + barrier, summed over the loop */
#define NRPN_SW_WAIT_MAX 23 /* ... and the longest one */
#define NRPN_SW_KSTEP0 24   /* conv: shader cycles at the end of each of the first 8 K-steps (0 = not executed) */

/* conv phases */
#define NRPN_SP_ENTRY 0
#define NRPN_SP_PROLOGUE_END 1 /* row addresses / tap masks / descriptors done, nothing loaded yet */
#define NRPN_SP_FIRST_TILE 2   /* first operand tile landed in LDS (its vmcnt(0) + barrier passed) */
#define NRPN_SP_LOOP_END 3
#define NRPN_SP_STORES_ISSUED 4
#define NRPN_SP_STORES_DONE 5  /* after wave 0's s_waitcnt vmcnt(0) */
#define NRPN_SP_EXIT 6
#define NRPN_SP_CONV_PHASES 7
/* epilogue phases */
#define NRPN_SE_ENTRY 0
#define NRPN_SE_FIRST_LOADS 1  /* the partials of lane 0's first element are back */
#define NRPN_SE_LAST_STORE 2
#define NRPN_SE_STORES_DONE 3
#define NRPN_SE_EXIT 4
#define NRPN_SE_PHASES 5

typedef struct nrpn_stamp_layout {
  int32_t words;            /* = NRPN_STAMP_WORDS */
  int32_t plan_code;        /* = nrpn_conv3d_fwd_plan_ex for the same arguments */
  int64_t conv_records;     /* workgroups of the conv launch */
  int64_t epilogue_records; /* workgroups of the epilogue launch, 0 when the plan has no K slices */
  int64_t bytes;            /* (conv_records + epilogue_records) * words * 8 */
  int32_t m_tiles, n_tiles, k_slices; /* ranges of the records' tile / slice ids (k_slices = 1: not sliced) */
  int32_t k_steps;          /* 128-byte K-steps of the whole GEMM */
  int32_t slice_steps[NRPN_STAMP_MAX_SLICES]; /* K-steps of slice z, z < k_slices */
} nrpn_stamp_layout;

/* Host only.  NRPN_ERR_ARG (message names the plan code) when the plan of this call has no stamped form: anything but bf16 in the
 * LDS-DMA kernels with the 128-byte K-step on the 128-row or the 8-wave 256x256 tile (plan codes 0..3 without a tail split). */
int nrpn_conv3d_fwd_stamp_layout(int n, int gx, int gy, int gz, int cin, int cout, int ksize, int dtype, const nrpn_conv_opts *opts,
                                 nrpn_stamp_layout *layout);
/* nrpn_conv3d_fwd_ex + stamps.  NRPN_ERR_ARG before anything is launched when stamps is null, stamps_bytes is below the layout's,
 * opts->debug != 0, statistics are requested or the plan has no stamped form. */
int nrpn_conv3d_fwd_stamped(const void *x, const void *wp, const float *bias, void *y, int n, int gx, int gy, int gz, int cin, int cout,
                            int wrows, int ksize, int dtype, int flags, void *workspace, const nrpn_conv_opts *opts,
                            nrpn_stream_t stream, uint64_t *stamps, size_t stamps_bytes);

#ifdef __cplusplus
}
#endif
#endif
