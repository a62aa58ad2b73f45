// valu_issue.hip -- issue cost of single VALU instructions on gfx950, measured two ways at 1 / 2 / 4 / 8 waves per SIMD:
//   (a) in-kernel: s_memtime around the stream (shader-clock ticks), lane 0 of every wave, averaged  -> cycles per
//       instruction as ONE wave sees them (at w waves per SIMD a wave gets 1/w of the SIMD: SIMD cost = that / w);
//   (b) wall: HIP events around the launch, converted at the NOMINAL 2.4 GHz -> cycles per instruction and SIMD;
//   and their quotient = the clock the chip actually held (ticks per second), so that neither figure rests on an assumed
//   frequency.
// Every stream is inline asm over 8 rotating registers (no instruction reads the result of the one before it), so the
// compiler can neither fold nor reorder anything, and every launch runs >= 5 ms so that launch overhead is < 1 %.
// Replaces the folded rows of profiles/r01_valu_rate_microbench.txt.
//   hipcc --offload-arch=gfx950 -O2 -o tools/valu_issue tools/valu_issue.hip && tools/valu_issue
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#define N_ITER 60000
#define UNR 32
#define BODY(txt, T)                                                                                                   \
    T a[8];                                                                                                            \
    for (int i = 0; i < 8; ++i) a[i] = (T)(threadIdx.x * 3 + i + seed);                                                \
    unsigned long long t0, t1;                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");               \
    for (int it = 0; it < N_ITER; ++it) {                                                                              \
        _Pragma("unroll") for (int u = 0; u < UNR; ++u) {                                                              \
            const int i = u & 7;                                                                                       \
            asm volatile(txt : "=v"(a[i]) : "v"(a[(i + 3) & 7]), "v"(a[(i + 1) & 7]), "v"(a[(i + 2) & 7]));            \
        }                                                                                                              \
    }                                                                                                                  \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");               \
    T r = 0;                                                                                                           \
    for (int i = 0; i < 8; ++i) r += a[i];                                                                             \
    out[blockIdx.x * 64 + threadIdx.x] = (int)r;                                                                       \
    if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0;
#define OP(name, txt) \
    __global__ __launch_bounds__(64) void name(int* out, unsigned long long* ticks, int seed) { BODY(txt, int) }
#define OP64(name, txt) \
    __global__ __launch_bounds__(64) void name(int* out, unsigned long long* ticks, int seed) { BODY(txt, long long) }

OP(k_fma, "v_fma_f32 %0, %1, %2, %3")
OP64(k_pkfma, "v_pk_fma_f32 %0, %1, %2, %3")
OP64(k_pkadd32, "v_pk_add_f32 %0, %1, %2")
OP(k_mulf, "v_mul_f32 %0, %1, %2")
OP(k_addf, "v_add_f32 %0, %1, %2")
OP(k_maxf, "v_max_f32 %0, %1, %2")
OP(k_max3f, "v_max3_f32 %0, %1, %2, %3")
OP(k_max3i, "v_max3_i32 %0, %1, %2, %3")
OP(k_maxi, "v_max_i32 %0, %1, %2")
OP(k_maxi16, "v_max_i16 %0, %1, %2")
OP(k_maxu16, "v_max_u16 %0, %1, %2")
OP(k_add, "v_add_u32 %0, %1, %2")
OP(k_addc, "v_add_i32 %0, %1, %2 clamp")
OP(k_subc, "v_sub_u32_e64 %0, %1, %2 clamp")
OP(k_and, "v_and_b32 %0, %1, %2")
OP(k_or, "v_or_b32 %0, %1, %2")
OP(k_xor, "v_xor_b32 %0, %1, %2")
OP(k_mov, "v_mov_b32 %0, %2")
OP(k_sdwa, "v_add_u32_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1")
OP(k_perm, "v_perm_b32 %0, %1, %2, %3")
OP(k_dot4i8, "v_dot4_i32_i8 %0, %1, %2, %3")
OP(k_dot4u8, "v_dot4_u32_u8 %0, %1, %2, %3")
OP(k_dot8i4, "v_dot8_i32_i4 %0, %1, %2, %3")
OP(k_dot2i16, "v_dot2_i32_i16 %0, %1, %2, %3")
OP(k_sad8, "v_sad_u8 %0, %1, %2, %3")
OP(k_bfei, "v_bfe_i32 %0, %1, 8, 8")
OP(k_pkmax, "v_pk_max_i16 %0, %1, %2")
OP(k_pkadd, "v_pk_add_i16 %0, %1, %2")
OP(k_pksubc, "v_pk_sub_u16 %0, %1, %2 clamp")
OP(k_cndmask, "v_cndmask_b32_e64 %0, %1, %2, s[2:3]")   // the kernarg pointer pair as an arbitrary lane mask
OP(k_cmp, "v_cmp_eq_u32 vcc, %1, %2\n\tv_mov_b32 %0, %3")   // a compare needs a VGPR result to stay in the rotation: 2 instructions
OP(k_lshl, "v_lshlrev_b32 %0, 3, %1")
OP(k_lshladd, "v_lshl_add_u32 %0, %1, 2, %2")
OP(k_add3, "v_add3_u32 %0, %1, %2, %3")
OP(k_mad24, "v_mad_i32_i24 %0, %1, %2, %3")
OP(k_cvtub, "v_cvt_f32_ubyte1 %0, %1")
OP(k_dpp, "v_mov_b32_dpp %0, %2 wave_shr:1 row_mask:0xf bank_mask:0xf")
OP(k_adddpp, "v_add_u32_dpp %0, %1, %2 row_shr:1 row_mask:0xf bank_mask:0xf")
OP(k_max3i16, "v_max3_i16 %0, %1, %2, %3")
OP(k_max3u16, "v_max3_u16 %0, %1, %2, %3")
OP(k_min3i16, "v_min3_i16 %0, %1, %2, %3")
OP(k_med3i16, "v_med3_i16 %0, %1, %2, %3")
OP(k_addu16, "v_add_u16 %0, %1, %2")
OP(k_subu16c, "v_sub_u16_e64 %0, %1, %2 clamp")
OP(k_addi16c, "v_add_i16 %0, %1, %2 clamp")
OP(k_madu16, "v_mad_u16 %0, %1, %2, %3")
OP(k_max3f16, "v_max3_f16 %0, %1, %2, %3")
OP(k_maxf16, "v_max_f16 %0, %1, %2")
OP(k_addu16sdwa, "v_add_u16_sdwa %0, %1, sext(%2) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1")
OP(k_addcou32, "v_addc_co_u32 %0, vcc, %1, %2, vcc")
OP(k_subrev, "v_subrev_u32 %0, %1, %2")
OP(k_bfi2, "v_bfi_b32 %0, %1, %2, %3")
OP(k_andor, "v_and_or_b32 %0, %1, %2, %3")
// VGPR index mode (the profile form of the batched kernels): 4 indexed full-rate adds between one s_set_gpr_idx_on / _off pair,
// and the VALU of four SW cells (4 adds + 6 max3 + 4 sub-clamp) with the pair and one s_bfe -- against the table form's
// (4 sdwa adds + xor + perm + the same).  Counted per CELL.  (Scalar temporaries are compiler-allocated operands, m0 is declared.)
#define BODY_X(txt)                                                                                                    \
    int a[8];                                                                                                          \
    for (int i = 0; i < 8; ++i) a[i] = threadIdx.x * 3 + i + seed;                                                     \
    int st = seed;                                                                                                     \
    unsigned long long t0, t1;                                                                                         \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");               \
    for (int it = 0; it < N_ITER; ++it) {                                                                              \
        _Pragma("unroll") for (int u = 0; u < UNR / 4; ++u) {                                                          \
            const int i = u & 7;                                                                                       \
            asm volatile(txt : "=&v"(a[i]), "+s"(st) : "v"(a[(i + 3) & 7]), "v"(a[(i + 1) & 7]), "v"(a[(i + 2) & 7]) : "m0", "scc"); \
        }                                                                                                              \
    }                                                                                                                  \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");               \
    int r = st;                                                                                                        \
    for (int i = 0; i < 8; ++i) r += a[i];                                                                             \
    out[blockIdx.x * 64 + threadIdx.x] = r;                                                                            \
    if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0;
#define OPX(name, txt) \
    __global__ __launch_bounds__(64) void name(int* out, unsigned long long* ticks, int seed) { BODY_X(txt) }
OPX(k_idx4, "s_set_gpr_idx_on 0, 1\n\tv_add_u32 %0, %2, %3\n\tv_add_u32 %0, %2, %4\n\tv_add_u32 %0, %3, %4\n\tv_add_u32 %0, %4, %3\n\ts_set_gpr_idx_off")
OPX(k_cell4, "s_bfe_u32 %1, %1, 0x80008\n\ts_set_gpr_idx_on 0, 1\n\tv_add_u32 %0, %2, %3\n\tv_add_u32 %0, %2, %4\n\tv_add_u32 %0, %3, %4\n\tv_add_u32 %0, %4, %3\n\ts_set_gpr_idx_off\n\tv_max3_i32 %0, %2, %3, %4\n\tv_sub_u32_e64 %0, %2, %3 clamp\n\tv_max3_i32 %0, %2, %3, %4\n\tv_sub_u32_e64 %0, %2, %4 clamp\n\tv_max3_i32 %0, %4, %3, %2\n\tv_sub_u32_e64 %0, %3, %2 clamp\n\tv_max3_i32 %0, %2, %4, %3\n\tv_sub_u32_e64 %0, %4, %2 clamp\n\tv_max3_i32 %0, %3, %4, %2\n\tv_max3_i32 %0, %3, %2, %4")
OPX(k_cell4old, "v_add_u32_sdwa %0, %2, sext(%3) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\tv_add_u32_sdwa %0, %2, sext(%4) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\tv_add_u32_sdwa %0, %3, sext(%4) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\tv_add_u32_sdwa %0, %4, sext(%3) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3\n\tv_xor_b32 %0, %2, %3\n\tv_perm_b32 %0, %2, %3, %4\n\tv_max3_i32 %0, %2, %3, %4\n\tv_sub_u32_e64 %0, %2, %3 clamp\n\tv_max3_i32 %0, %2, %3, %4\n\tv_sub_u32_e64 %0, %2, %4 clamp\n\tv_max3_i32 %0, %4, %3, %2\n\tv_sub_u32_e64 %0, %3, %2 clamp\n\tv_max3_i32 %0, %2, %4, %3\n\tv_sub_u32_e64 %0, %4, %2 clamp\n\tv_max3_i32 %0, %3, %4, %2\n\tv_max3_i32 %0, %3, %2, %4")
// packed f16 / u16 forms of the SW cell (two pairs per lane; r04)
OP(k_pkmaximum3f16, "v_pk_maximum3_f16 %0, %1, %2, %3")
OP(k_pkaddf16, "v_pk_add_f16 %0, %1, %2")
OP(k_pkaddf16c, "v_pk_add_f16 %0, %1, %2 clamp")
OP(k_pkmaxf16, "v_pk_max_f16 %0, %1, %2")
OP(k_pkaddu16, "v_pk_add_u16 %0, %1, %2")
OP(k_permsgpr, "v_perm_b32 %0, s2, %2, %3")   // the kernarg pointer's low word as an arbitrary SGPR table half
OPX(k_cell16, "v_perm_b32 %0, s2, %2, %3\n\tv_pk_add_f16 %0, %3, %4\n\tv_pk_maximum3_f16 %0, %2, %3, %4\n\tv_pk_add_f16 %0, %2, %4 clamp\n\tv_perm_b32 %0, s2, %3, %4\n\tv_pk_add_f16 %0, %2, %4\n\tv_pk_maximum3_f16 %0, %3, %2, %4\n\tv_pk_add_f16 %0, %3, %4 clamp\n\tv_pk_maximum3_f16 %0, %4, %3, %2")
// packed f16 profile form (r05 step 0): ONE wave-uniform pattern row against 128 texts, one row step over a block of C columns.
// The profile (4 codes + a pad register per column, 5C VGPRs) is pinned at v32.., the row's code x C is an SGPR, and the C
// diagonal adds read it through index mode (SRC1) -- or, in the movrels row, through one v_movrels_b32 per column (M0 = code x C).
// Then per column the chain h = max3(t', G_up, G_left), G = h + g, and half a running-best max3; one v_mov hands the block's last
// G to the next block.  All registers are physical (clobbered), so the compiler only supplies the loop.  Counted per CELL (2C per step).
#define PROF_CLOBBERS "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107"
#define OPP(name, txt)                                                                                                 \
    __global__ __launch_bounds__(64) void name(int* out, unsigned long long* ticks, int seed) {                        \
        int st = 0;                                                                                                    \
        asm volatile("v_mov_b32 v32, 0x10001000\n\tv_mov_b32 v33, 0x10401040\n\tv_mov_b32 v34, 0x10801080\n\tv_mov_b32 v35, 0x10c010c0\n\tv_mov_b32 v36, 0x11001100\n\tv_mov_b32 v37, 0x11401140\n\tv_mov_b32 v38, 0x11801180\n\tv_mov_b32 v39, 0x11c011c0\n\tv_mov_b32 v40, 0x10001000\n\tv_mov_b32 v41, 0x10401040\n\tv_mov_b32 v42, 0x10801080\n\tv_mov_b32 v43, 0x10c010c0\n\tv_mov_b32 v44, 0x11001100\n\tv_mov_b32 v45, 0x11401140\n\tv_mov_b32 v46, 0x11801180\n\tv_mov_b32 v47, 0x11c011c0\n\tv_mov_b32 v48, 0x10001000\n\tv_mov_b32 v49, 0x10401040\n\tv_mov_b32 v50, 0x10801080\n\tv_mov_b32 v51, 0x10c010c0\n\tv_mov_b32 v52, 0x11001100\n\tv_mov_b32 v53, 0x11401140\n\tv_mov_b32 v54, 0x11801180\n\tv_mov_b32 v55, 0x11c011c0\n\tv_mov_b32 v56, 0x10001000\n\tv_mov_b32 v57, 0x10401040\n\tv_mov_b32 v58, 0x10801080\n\tv_mov_b32 v59, 0x10c010c0\n\tv_mov_b32 v60, 0x11001100\n\tv_mov_b32 v61, 0x11401140\n\tv_mov_b32 v62, 0x11801180\n\tv_mov_b32 v63, 0x11c011c0\n\tv_mov_b32 v64, 0x10001000\n\tv_mov_b32 v65, 0x10401040\n\tv_mov_b32 v66, 0x10801080\n\tv_mov_b32 v67, 0x10c010c0\n\tv_mov_b32 v68, 0x11001100\n\tv_mov_b32 v69, 0x11401140\n\tv_mov_b32 v70, 0x11801180\n\tv_mov_b32 v71, 0x11c011c0\n\tv_mov_b32 v72, 0x10001000\n\tv_mov_b32 v73, 0x10401040\n\tv_mov_b32 v74, 0x10801080\n\tv_mov_b32 v75, 0x10c010c0\n\tv_mov_b32 v76, 0x11001100\n\tv_mov_b32 v77, 0x11401140\n\tv_mov_b32 v78, 0x11801180\n\tv_mov_b32 v79, 0x11c011c0\n\tv_mov_b32 v80, 0x10001000\n\tv_mov_b32 v81, 0x10401040\n\tv_mov_b32 v82, 0x10801080\n\tv_mov_b32 v83, 0x10c010c0\n\tv_mov_b32 v84, 0x11001100\n\tv_mov_b32 v85, 0x11401140\n\tv_mov_b32 v86, 0x11801180\n\tv_mov_b32 v87, 0x11c011c0\n\tv_mov_b32 v88, 0x10001000\n\tv_mov_b32 v89, 0x10401040\n\tv_mov_b32 v90, 0x10801080\n\tv_mov_b32 v91, 0x10c010c0\n\tv_mov_b32 v92, 0x11001100\n\tv_mov_b32 v93, 0x11401140\n\tv_mov_b32 v94, 0x11801180\n\tv_mov_b32 v95, 0x11c011c0\n\tv_mov_b32 v96, 0x10001000\n\tv_mov_b32 v97, 0x10401040\n\tv_mov_b32 v98, 0x10801080\n\tv_mov_b32 v99, 0x10c010c0\n\tv_mov_b32 v100, 0x11001100\n\tv_mov_b32 v101, 0x11401140\n\tv_mov_b32 v102, 0x11801180\n\tv_mov_b32 v103, 0x11c011c0\n\tv_mov_b32 v104, 0x10001000\n\tv_mov_b32 v105, 0x10401040\n\tv_mov_b32 v106, 0x10801080\n\tv_mov_b32 v107, 0x10c010c0" ::: PROF_CLOBBERS);                                                                          \
        unsigned long long t0, t1;                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");           \
        for (int it = 0; it < N_ITER; ++it) {                                                                          \
            _Pragma("unroll") for (int u = 0; u < UNR / 4; ++u) asm volatile(txt : "+s"(st) : : PROF_CLOBBERS, "m0", "scc"); \
        }                                                                                                              \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");           \
        int r;                                                                                                         \
        asm volatile("v_mov_b32 %0, v103" : "=v"(r) : : PROF_CLOBBERS);                                               \
        out[blockIdx.x * 64 + threadIdx.x] = r + st + seed;                                                            \
        if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0;                                                             \
    }
OPP(k_prof8, "s_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_pk_add_f16 v80, v100, v32 clamp\n\tv_pk_add_f16 v81, v72, v33 clamp\n\tv_pk_add_f16 v82, v73, v34 clamp\n\tv_pk_add_f16 v83, v74, v35 clamp\n\tv_pk_add_f16 v84, v75, v36 clamp\n\tv_pk_add_f16 v85, v76, v37 clamp\n\tv_pk_add_f16 v86, v77, v38 clamp\n\tv_pk_add_f16 v87, v78, v39 clamp\n\ts_set_gpr_idx_off\n\tv_pk_maximum3_f16 v88, v80, v72, v101\n\tv_pk_add_f16 v72, v88, v102\n\tv_pk_maximum3_f16 v89, v81, v73, v72\n\tv_pk_add_f16 v73, v89, v102\n\tv_pk_maximum3_f16 v90, v82, v74, v73\n\tv_pk_add_f16 v74, v90, v102\n\tv_pk_maximum3_f16 v91, v83, v75, v74\n\tv_pk_add_f16 v75, v91, v102\n\tv_pk_maximum3_f16 v92, v84, v76, v75\n\tv_pk_add_f16 v76, v92, v102\n\tv_pk_maximum3_f16 v93, v85, v77, v76\n\tv_pk_add_f16 v77, v93, v102\n\tv_pk_maximum3_f16 v94, v86, v78, v77\n\tv_pk_add_f16 v78, v94, v102\n\tv_pk_maximum3_f16 v95, v87, v79, v78\n\tv_pk_add_f16 v79, v95, v102\n\tv_pk_maximum3_f16 v103, v103, v88, v89\n\tv_pk_maximum3_f16 v104, v104, v90, v91\n\tv_pk_maximum3_f16 v105, v105, v92, v93\n\tv_pk_maximum3_f16 v106, v106, v94, v95\n\tv_mov_b32 v101, v79")
OPP(k_prof4, "s_add_u32 %0, %0, 4\n\ts_and_b32 %0, %0, 15\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_pk_add_f16 v80, v100, v32 clamp\n\tv_pk_add_f16 v81, v72, v33 clamp\n\tv_pk_add_f16 v82, v73, v34 clamp\n\tv_pk_add_f16 v83, v74, v35 clamp\n\ts_set_gpr_idx_off\n\tv_pk_maximum3_f16 v88, v80, v72, v101\n\tv_pk_add_f16 v72, v88, v102\n\tv_pk_maximum3_f16 v89, v81, v73, v72\n\tv_pk_add_f16 v73, v89, v102\n\tv_pk_maximum3_f16 v90, v82, v74, v73\n\tv_pk_add_f16 v74, v90, v102\n\tv_pk_maximum3_f16 v91, v83, v75, v74\n\tv_pk_add_f16 v75, v91, v102\n\tv_pk_maximum3_f16 v103, v103, v88, v89\n\tv_pk_maximum3_f16 v104, v104, v90, v91\n\tv_mov_b32 v101, v75")
// integer-coded profile form: H stored as the integer k in each half, v_pk_maximum3_f16 only orders.  8 indexed v_add_u32 (one 32-bit add
// for both halves), 8 max3, 8 v_pk_sub_u16 clamp, 4 best max3; no v_mov -- the last column's subtract writes the row's col register, which
// the next row reads as its column-7 up (two row steps per asm text, v101 / v107 alternating as col[r] / col[r + 1])
OPP(k_prof8i, "s_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v100, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_maximum3_f16 v88, v80, v72, v101\n\tv_pk_sub_u16 v72, v88, v102 clamp\n\tv_pk_maximum3_f16 v89, v81, v73, v72\n\tv_pk_sub_u16 v73, v89, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v88, v89\n\tv_pk_maximum3_f16 v90, v82, v74, v73\n\tv_pk_sub_u16 v74, v90, v102 clamp\n\tv_pk_maximum3_f16 v91, v83, v75, v74\n\tv_pk_sub_u16 v75, v91, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v90, v91\n\tv_pk_maximum3_f16 v92, v84, v76, v75\n\tv_pk_sub_u16 v76, v92, v102 clamp\n\tv_pk_maximum3_f16 v93, v85, v77, v76\n\tv_pk_sub_u16 v77, v93, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v92, v93\n\tv_pk_maximum3_f16 v94, v86, v78, v77\n\tv_pk_sub_u16 v78, v94, v102 clamp\n\tv_pk_maximum3_f16 v95, v87, v107, v78\n\tv_pk_sub_u16 v101, v95, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v94, v95\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v100, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_maximum3_f16 v88, v80, v72, v107\n\tv_pk_sub_u16 v72, v88, v102 clamp\n\tv_pk_maximum3_f16 v89, v81, v73, v72\n\tv_pk_sub_u16 v73, v89, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v88, v89\n\tv_pk_maximum3_f16 v90, v82, v74, v73\n\tv_pk_sub_u16 v74, v90, v102 clamp\n\tv_pk_maximum3_f16 v91, v83, v75, v74\n\tv_pk_sub_u16 v75, v91, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v90, v91\n\tv_pk_maximum3_f16 v92, v84, v76, v75\n\tv_pk_sub_u16 v76, v92, v102 clamp\n\tv_pk_maximum3_f16 v93, v85, v77, v76\n\tv_pk_sub_u16 v77, v93, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v92, v93\n\tv_pk_maximum3_f16 v94, v86, v78, v77\n\tv_pk_sub_u16 v78, v94, v102 clamp\n\tv_pk_maximum3_f16 v95, v87, v101, v78\n\tv_pk_sub_u16 v107, v95, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v94, v95")
// the integer row in the kernel's true shape (batch_scores.hip.h, INT = true): the last column's subtract is deferred into the next row's step
// and writes the row's col register in place after the next row has read it as its diagonal (v101 = the pending m), two rows to a kernel asm
// text with the pad test (s_cmp + a never-taken branch) behind the pair's first adds.  Two pairs per text here: the col registers
// v96..v99 stand for col[r - 1 .. r + 2] and come round after four rows, which 152 distinct registers do not need to.
OPP(k_prof8n, "s_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v99, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v99, v101, v102 clamp\n\ts_cmp_eq_u32 %0, 32\n\ts_cbranch_scc1 .Lpad%=\n\tv_pk_maximum3_f16 v80, v80, v72, v96\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v99, v78\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v96, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v96, v101, v102 clamp\n\tv_pk_maximum3_f16 v80, v80, v72, v97\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v96, v78\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\t.Lpad%=:\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v97, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v97, v101, v102 clamp\n\ts_cmp_eq_u32 %0, 32\n\ts_cbranch_scc1 .Lpbd%=\n\tv_pk_maximum3_f16 v80, v80, v72, v98\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v97, v78\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v80, v98, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v98, v101, v102 clamp\n\tv_pk_maximum3_f16 v80, v80, v72, v99\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v98, v78\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\t.Lpbd%=:")
// ... and the same row split into two independent half-chains ("skew"): a step runs row r's columns 4..7 against row r + 1's columns
// 0..3, interleaved instruction by instruction, so the dependent chain is 8 long instead of 16.  All eight adds sit under one
// s_set_gpr_idx_on, row r's three (columns 5..7) first, then s_set_gpr_idx_idx to row r + 1's offset for its four and for column 4's add
// of the NEXT step (it needs H(r, 3) before row r + 1 overwrites it: one more live register, v84 / v88 alternating).  28 VALU per step
// of 16 cells as the nomove row, the same two scalar instructions per row and the same pad test per two rows; four steps per text.
OPP(k_prof8s, "s_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_idx %0\n\tv_add_u32 v80, v96, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v88, v75, v36\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v99, v101, v102 clamp\n\ts_cmp_eq_u32 %0, 32\n\ts_cbranch_scc1 .Lskw0_%=\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_maximum3_f16 v80, v80, v72, v97\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v99, v78\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\t.Lskw0_%=:\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_idx %0\n\tv_add_u32 v80, v97, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v96, v101, v102 clamp\n\tv_pk_maximum3_f16 v88, v88, v76, v75\n\tv_pk_maximum3_f16 v80, v80, v72, v98\n\tv_pk_sub_u16 v76, v88, v102 clamp\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v88, v85\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v96, v78\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_idx %0\n\tv_add_u32 v80, v98, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v88, v75, v36\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v97, v101, v102 clamp\n\ts_cmp_eq_u32 %0, 32\n\ts_cbranch_scc1 .Lskw2_%=\n\tv_pk_maximum3_f16 v84, v84, v76, v75\n\tv_pk_maximum3_f16 v80, v80, v72, v99\n\tv_pk_sub_u16 v76, v84, v102 clamp\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v84, v85\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v97, v78\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\tv_pk_maximum3_f16 v104, v104, v82, v83\n\t.Lskw2_%=:\n\ts_set_gpr_idx_on %0, gpr_idx(SRC1)\n\tv_add_u32 v85, v76, v37\n\tv_add_u32 v86, v77, v38\n\tv_add_u32 v87, v78, v39\n\ts_add_u32 %0, %0, 8\n\ts_and_b32 %0, %0, 31\n\ts_set_gpr_idx_idx %0\n\tv_add_u32 v80, v99, v32\n\tv_add_u32 v81, v72, v33\n\tv_add_u32 v82, v73, v34\n\tv_add_u32 v83, v74, v35\n\tv_add_u32 v84, v75, v36\n\ts_set_gpr_idx_off\n\tv_pk_sub_u16 v98, v101, v102 clamp\n\tv_pk_maximum3_f16 v88, v88, v76, v75\n\tv_pk_maximum3_f16 v80, v80, v72, v96\n\tv_pk_sub_u16 v76, v88, v102 clamp\n\tv_pk_sub_u16 v72, v80, v102 clamp\n\tv_pk_maximum3_f16 v85, v85, v77, v76\n\tv_pk_maximum3_f16 v81, v81, v73, v72\n\tv_pk_sub_u16 v77, v85, v102 clamp\n\tv_pk_sub_u16 v73, v81, v102 clamp\n\tv_pk_maximum3_f16 v105, v105, v88, v85\n\tv_pk_maximum3_f16 v103, v103, v80, v81\n\tv_pk_maximum3_f16 v86, v86, v78, v77\n\tv_pk_maximum3_f16 v82, v82, v74, v73\n\tv_pk_sub_u16 v78, v86, v102 clamp\n\tv_pk_sub_u16 v74, v82, v102 clamp\n\tv_pk_maximum3_f16 v101, v87, v98, v78\n\tv_pk_maximum3_f16 v83, v83, v75, v74\n\tv_pk_sub_u16 v75, v83, v102 clamp\n\tv_pk_maximum3_f16 v106, v106, v86, v101\n\tv_pk_maximum3_f16 v104, v104, v82, v83")
// (a v_movrels_b32 variant, one per column with M0 = code x C, does not exist here: gfx950 has no v_movrel* -- the assembler
// rejects it as "instruction not supported on this GPU"; index mode is the only indexed VGPR read)
OP(k_nop, "s_nop 0")

// dependent chains (every instruction reads the result of the one before it) and chains diluted with independent fillers:
// what ONE wave alone on its SIMD sustains -- the single-pair fill kernel's regime (one stripe = one wave per SIMD)
#define OPDEP(name, txt) \
    __global__ __launch_bounds__(64) void name(int* out, unsigned long long* ticks, int seed) { \
        int a[8]; for (int i = 0; i < 8; ++i) a[i] = threadIdx.x * 3 + i + seed; \
        unsigned long long t0, t1; \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory"); \
        for (int it = 0; it < N_ITER; ++it) { _Pragma("unroll") for (int u = 0; u < UNR / 4; ++u) { \
            asm volatile(txt : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]) : "v"(a[6]), "v"(a[7])); } } \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory"); \
        int r = 0; for (int i = 0; i < 8; ++i) r += a[i]; out[blockIdx.x * 64 + threadIdx.x] = r; \
        if (threadIdx.x == 0) ticks[blockIdx.x] = t1 - t0; }
// %0 is the chain register; %1..%5 are filler registers; %6, %7 read-only.  Each macro body = 4 chain instructions (+ fillers).
OPDEP(d_add, "v_add_u32 %0, %0, %6\n\tv_add_u32 %0, %0, %7\n\tv_add_u32 %0, %0, %6\n\tv_add_u32 %0, %0, %7")
OPDEP(d_and, "v_and_b32 %0, %0, %6\n\tv_or_b32 %0, %0, %7\n\tv_and_b32 %0, %0, %6\n\tv_or_b32 %0, %0, %7")
OPDEP(d_max3, "v_max3_i32 %0, %0, %6, %7\n\tv_max3_i32 %0, %0, %7, %6\n\tv_max3_i32 %0, %0, %6, %7\n\tv_max3_i32 %0, %0, %7, %6")
OPDEP(d_sdwa, "v_add_u32_sdwa %0, %0, sext(%6) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\tv_add_u32_sdwa %0, %0, sext(%7) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\tv_add_u32_sdwa %0, %0, sext(%6) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1\n\tv_add_u32_sdwa %0, %0, sext(%7) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1")
OPDEP(d_dpp, "v_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf")
// the fill kernel's chain: max3 -> and -> add, undiluted; then with one / two independent fillers after every chain instruction
OPDEP(d_mix, "v_max3_i32 %0, %0, %6, %7\n\tv_and_b32 %0, %0, %6\n\tv_add_u32 %0, %0, %7\n\tv_max3_i32 %0, %0, %7, %6")
OPDEP(d_mix1, "v_max3_i32 %0, %0, %6, %7\n\tv_add_u32 %1, %1, %6\n\tv_and_b32 %0, %0, %6\n\tv_add_u32 %2, %2, %6\n\tv_add_u32 %0, %0, %7\n\tv_add_u32 %3, %3, %6\n\tv_max3_i32 %0, %0, %7, %6\n\tv_add_u32 %4, %4, %6")
OPDEP(d_mix1s, "v_max3_i32 %0, %0, %6, %7\n\tv_perm_b32 %1, %1, %6, %7\n\tv_and_b32 %0, %0, %6\n\tv_perm_b32 %2, %2, %6, %7\n\tv_add_u32 %0, %0, %7\n\tv_perm_b32 %3, %3, %6, %7\n\tv_max3_i32 %0, %0, %7, %6\n\tv_perm_b32 %4, %4, %6, %7")
OPDEP(d_mix2, "v_max3_i32 %0, %0, %6, %7\n\tv_add_u32 %1, %1, %6\n\tv_add_u32 %5, %5, %6\n\tv_and_b32 %0, %0, %6\n\tv_add_u32 %2, %2, %6\n\tv_add_u32 %1, %1, %7\n\tv_add_u32 %0, %0, %7\n\tv_add_u32 %3, %3, %6\n\tv_add_u32 %2, %2, %7\n\tv_max3_i32 %0, %0, %7, %6\n\tv_add_u32 %4, %4, %6\n\tv_add_u32 %3, %3, %7")

typedef void (*kfn)(int*, unsigned long long*, int);
int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : nullptr;   // run only the rows whose name contains this
    struct { const char* n; kfn f; int per; } t[] = {
        {"v_fma_f32", k_fma, 1}, {"v_pk_fma_f32", k_pkfma, 1}, {"v_pk_add_f32", k_pkadd32, 1}, {"v_mul_f32", k_mulf, 1}, {"v_add_f32", k_addf, 1},
        {"v_max_f32", k_maxf, 1}, {"v_max3_f32", k_max3f, 1}, {"v_max3_i32", k_max3i, 1}, {"v_max_i32", k_maxi, 1}, {"v_max_i16", k_maxi16, 1},
        {"v_max_u16", k_maxu16, 1}, {"v_add_u32", k_add, 1}, {"v_add_i32 clamp", k_addc, 1}, {"v_sub_u32 clamp", k_subc, 1}, {"v_and_b32", k_and, 1},
        {"v_or_b32", k_or, 1}, {"v_xor_b32", k_xor, 1}, {"v_mov_b32", k_mov, 1}, {"v_add_u32_sdwa sext(byte)", k_sdwa, 1}, {"v_perm_b32", k_perm, 1},
        {"v_pk_max_i16", k_pkmax, 1}, {"v_pk_add_i16", k_pkadd, 1}, {"v_pk_sub_u16 clamp", k_pksubc, 1}, {"v_cndmask_b32 (sgpr mask)", k_cndmask, 1},
        {"v_cmp_eq_u32 + v_mov_b32", k_cmp, 2}, {"v_lshlrev_b32", k_lshl, 1}, {"v_lshl_add_u32", k_lshladd, 1}, {"v_add3_u32", k_add3, 1},
        {"v_mad_i32_i24", k_mad24, 1}, {"v_cvt_f32_ubyte1", k_cvtub, 1}, {"v_mov_b32_dpp wave_shr:1", k_dpp, 1}, {"v_add_u32_dpp row_shr:1", k_adddpp, 1},
        {"v_max3_i16", k_max3i16, 1}, {"v_max3_u16", k_max3u16, 1}, {"v_min3_i16", k_min3i16, 1}, {"v_med3_i16", k_med3i16, 1}, {"v_add_u16", k_addu16, 1},
        {"v_sub_u16 clamp", k_subu16c, 1}, {"v_add_i16 clamp", k_addi16c, 1}, {"v_mad_u16", k_madu16, 1}, {"v_max3_f16", k_max3f16, 1}, {"v_max_f16", k_maxf16, 1},
        {"v_add_u16_sdwa sext(byte)", k_addu16sdwa, 1}, {"v_addc_co_u32", k_addcou32, 1}, {"v_subrev_u32", k_subrev, 1}, {"v_bfi_b32", k_bfi2, 1},
        {"v_and_or_b32", k_andor, 1}, {"idx_on+4 v_add+idx_off /add", k_idx4, 1},
        {"v_dot4_i32_i8", k_dot4i8, 1}, {"v_dot4_u32_u8", k_dot4u8, 1}, {"v_dot8_i32_i4", k_dot8i4, 1}, {"v_dot2_i32_i16", k_dot2i16, 1},
        {"v_sad_u8", k_sad8, 1}, {"v_bfe_i32", k_bfei, 1},
        {"v_pk_maximum3_f16", k_pkmaximum3f16, 1}, {"v_pk_add_f16", k_pkaddf16, 1}, {"v_pk_add_f16 clamp", k_pkaddf16c, 1},
        {"v_pk_max_f16", k_pkmaxf16, 1}, {"v_pk_add_u16", k_pkaddu16, 1}, {"v_perm_b32 (sgpr table)", k_permsgpr, 1},
        {"SW cell16, 2 rows x 2 pairs /cell", k_cell16, 1},
        {"SW pk16 profile C=8 idx /cell", k_prof8, 4}, {"SW pk16 profile C=4 idx /cell", k_prof4, 2}, {"SW pk16 profile C=8 int /cell", k_prof8i, 8},
        {"SW pk16 profile C=8 int nomove /cell", k_prof8n, 16}, {"SW pk16 profile C=8 int skew /cell", k_prof8s, 16},
        {"SW cell, profile form /cell", k_cell4, 1}, {"SW cell, table form   /cell", k_cell4old, 1}, {"s_nop 0", k_nop, 1}};
    struct { const char* n; kfn f; int chain, total; } dt_[] = {
        {"v_add_u32 chain", d_add, 4, 4}, {"v_and/v_or chain", d_and, 4, 4}, {"v_max3_i32 chain", d_max3, 4, 4}, {"v_add_u32_sdwa chain", d_sdwa, 4, 4},
        {"v_mov_b32_dpp wave_shr chain", d_dpp, 4, 4}, {"max3->and->add chain", d_mix, 4, 4}, {"... + 1 v_add filler each", d_mix1, 4, 8},
        {"... + 1 v_perm filler each", d_mix1s, 4, 8}, {"... + 2 v_add fillers each", d_mix2, 4, 12}};
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int max_blocks = prop.multiProcessorCount * 4 * 8;
    int* d;
    unsigned long long* dt;
    hipMalloc(&d, (size_t)max_blocks * 64 * 4);
    hipMalloc(&dt, (size_t)max_blocks * 8);
    std::vector<unsigned long long> ht(max_blocks);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    printf("device %s, %d CUs.  Per instruction stream, at w = 1 / 2 / 4 / 8 waves per SIMD (every SIMD of the chip busy):\n", prop.gcnArchName,
           prop.multiProcessorCount);
    printf("  cyc/SIMD(ticks) = s_memtime ticks per instruction of one wave / w;  cyc/SIMD(wall@2.4) = wall time x 2.4 GHz per instruction / w ... and the\n"
           "  clock they imply (GHz = ticks / wall).  %d x %d instructions per wave and launch.\n", N_ITER, UNR);
    printf("%-28s | %-31s | %-31s | %s\n", "instruction", "cyc/SIMD (s_memtime ticks)", "cyc/SIMD (wall at 2.4 GHz)", "ms per launch (w=1), tick rate GHz (w=1, w=8)");
    for (auto& e : t) {
        if (only && !strstr(e.n, only)) continue;
        double ct[4], cw[4], ghz[4], ms1 = 0;
        int q = 0;
        for (int wps : {1, 2, 4, 8}) {
            const int blocks = prop.multiProcessorCount * 4 * wps;
            hipLaunchKernelGGL(e.f, dim3(blocks), dim3(64), 0, 0, d, dt, 3);
            hipDeviceSynchronize();
            hipEventRecord(e0);
            hipLaunchKernelGGL(e.f, dim3(blocks), dim3(64), 0, 0, d, dt, 3);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float ms;
            hipEventElapsedTime(&ms, e0, e1);
            hipMemcpy(ht.data(), dt, (size_t)blocks * 8, hipMemcpyDeviceToHost);
            double sum = 0;
            for (int b = 0; b < blocks; ++b) sum += (double)ht[b];
            const double n_instr = (double)N_ITER * UNR * e.per;
            ct[q] = sum / blocks / n_instr / wps;
            cw[q] = ms * 1e-3 * 2.4e9 / n_instr / wps;
            ghz[q] = (sum / blocks) / (ms * 1e-3) / 1e9;
            if (wps == 1) ms1 = ms;
            ++q;
        }
        fflush(stdout);
        printf("%-28s | %6.2f  %6.2f  %6.2f  %6.2f | %6.2f  %6.2f  %6.2f  %6.2f | %6.2f ms  %5.3f  %5.3f\n", e.n, ct[0], ct[1], ct[2], ct[3], cw[0], cw[1],
               cw[2], cw[3], ms1, ghz[0], ghz[3]);
    }
    printf("\nONE wave per SIMD (w = 1), dependent chains: cycles (s_memtime ticks) per CHAIN instruction, and per instruction overall\n");
    for (auto& e : dt_) {
        if (only) break;
        const int blocks = prop.multiProcessorCount * 4;
        hipLaunchKernelGGL(e.f, dim3(blocks), dim3(64), 0, 0, d, dt, 3);
        hipDeviceSynchronize();
        hipMemcpy(ht.data(), dt, (size_t)blocks * 8, hipMemcpyDeviceToHost);
        double sum = 0;
        for (int b = 0; b < blocks; ++b) sum += (double)ht[b];
        const double groups = (double)N_ITER * (UNR / 4);
        printf("%-32s | %6.2f per chain instruction | %6.2f per instruction (%d of %d on the chain)\n", e.n, sum / blocks / groups / e.chain,
               sum / blocks / groups / e.total, e.chain, e.total);
    }
    return 0;
}
