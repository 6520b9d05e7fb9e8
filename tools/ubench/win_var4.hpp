// win_var4.hpp -- A/B only: variants U, X, K of the product window loop
// (zrc4::win_windows) and their combinations, for tools/ubench/win_ubench.hip
// (modes 20-27).  One window is written once, ZW4_WINDOW, over
//   A  the register holding this window's &S[i_l] (its a_l read left from it),
//   N  the register that receives window n+1's &S[i_l],
//   C  the register the commit's S[i_l] = b_l write uses,
//   G  the filler of the last DPP gap (the v131 copy, or an s_nop),
//   X, K, Y  0 or 1, pasted into the piece names below.
//  U  the body twice per trip, (v106, v131) and (v131, v106): no copy of the
//     address, one taken branch per two windows; the first half leaves for
//     the drain on exit only.  Both registers hold the S base in bytes 1-3.
//  X  full-exec forms: every caller enters with all 64 lanes live, so exec is
//     restored with s_mov_b64 exec, -1 (no save), and the commit mask is a
//     v_cmp_lt_u32_e64 straight into s[46:47] (no s_and_b64).
//  K  byte masks as SDWA byte writes: J, d, x + 1 (variant S's three), t and
//     e.  The y' candidate and the ring slot move from under the b round trip
//     into the DPP gaps the t and e masks leave.  Every SDWA byte write has
//     one VALU op between it and its first reader.
//  Y  (K without X) the y mask folded into the select, v_cndmask_b32_sdwa
//     src0_sel:BYTE_0.  That form reads vcc, X's commit mask is in s[46:47]:
//     the two savings exclude each other.
// e (t - x - 1) lives in v119 here (free behind the duplicate-J select), so
// v131 can be an address register.
#pragma once
#include "../../zsummerx_amd/csrc/zrc4_win.hpp"
namespace zrc4 {

// J = scan + y', the b address and J's marker address
#define ZW4_J_0                                                                                    \
    "v_add_u32 v112, v112, v120\n\t"                                                               \
    "v_add_u32_sdwa v114, %[sb], v112 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t" \
    "v_and_b32 v112, 0xff, v112\n\t"
#define ZW4_J_1(SP)                                                                                \
    "v_add_u32_sdwa v112, v112, v120 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t" \
    SP                                                                                             \
    "v_add_u32 v114, %[sb], v112\n\t"
#define ZW4_JK_0(Y) ZW4_J_0
#define ZW4_JK_1(Y) ZW4_J_1(ZW4_JSP_##Y)
#define ZW4_JSP_0 "v_and_b32 %[y], 0xff, v120\n\t"
#define ZW4_JSP_1 "v_min_u32 v119, 16, %[rem]\n\t"

// window n-1's ring store
#define ZW4_RING_0                                                                                 \
    "s_mov_b64 s[40:41], exec\n\t"                                                                 \
    "s_mov_b64 exec, s[46:47]\n\t"                                                                 \
    "ds_write_b8 v125, v124\n\t"                                                                   \
    "s_mov_b64 exec, s[40:41]\n\t"
#define ZW4_RING_1                                                                                 \
    "s_mov_b64 exec, s[46:47]\n\t"                                                                 \
    "ds_write_b8 v125, v124\n\t"                                                                   \
    "s_mov_b64 exec, -1\n\t"

// d rule, rem cap, duplicate-J alternative (under the b / marker round trip)
#define ZW4_D_0(Y)                                                                                 \
    "v_and_b32 %[y], 0xff, v120\n\t"                                                               \
    "v_sub_u32 v118, v112, %[xa]\n\t"                                                              \
    "v_and_b32 v118, 0xff, v118\n\t"                                                               \
    "v_med3_u32 v119, v118, %[l], 16\n\t"                                                          \
    "v_cmp_ne_u32 vcc, v118, %[l]\n\t"                                                             \
    "v_cndmask_b32 v119, 16, v119, vcc\n\t"                                                        \
    "v_lshlrev_b32 v118, v119, 1\n\t"                                                              \
    "v_min_u32 v119, 16, %[rem]\n\t"                                                               \
    "v_lshlrev_b32 v119, v119, 1\n\t"                                                              \
    "v_or_b32 v118, v118, v119\n\t"                                                                \
    "v_or_b32 v119, v118, %[bitl]\n\t"                                                             \
    "v_or_b32 v130, %[l1], v112\n\t"                                                               \
    "v_bfi_b32 v125, %[rmask], %[rp], %[rb]\n\t"
#define ZW4_D_1(Y)                                                                                 \
    "v_sub_u32_sdwa v118, v112, %[xa] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t" \
    ZW4_DSP_##Y                                                                                    \
    "v_med3_u32 v129, v118, %[l], 16\n\t"                                                          \
    "v_cmp_ne_u32 vcc, v118, %[l]\n\t"                                                             \
    "v_cndmask_b32 v129, 16, v129, vcc\n\t"                                                        \
    "v_lshlrev_b32 v118, v129, 1\n\t"                                                              \
    ZW4_DSH_##Y                                                                                    \
    "v_or_b32 v118, v118, v119\n\t"                                                                \
    "v_or_b32 v119, v118, %[bitl]\n\t"
#define ZW4_DSP_0 "v_min_u32 v119, 16, %[rem]\n\t"
#define ZW4_DSH_0 "v_lshlrev_b32 v119, v119, 1\n\t"
#define ZW4_DSP_1 "v_lshlrev_b32 v119, v119, 1\n\t"
#define ZW4_DSH_1

// t, e and the gaps of the OR chain
#define ZW4_T_0 "v_add_u32 v128, v107, v116\n\t"
#define ZW4_T_1 "v_add_u32_sdwa v128, v107, v116 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
#define ZW4_G1_0                                                                                   \
    "v_sub_u32 v119, v128, %[xa]\n\t"                                                              \
    "v_and_b32 v128, 0xff, v128\n\t"
#define ZW4_G1_1                                                                                   \
    "v_or_b32 v130, %[l1], v112\n\t"                                                               \
    "v_sub_u32_sdwa v119, v128, %[xa] dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
#define ZW4_G2_0                                                                                   \
    "v_and_b32 v119, 0xff, v119\n\t"                                                               \
    "v_lshl_add_u32 v129, v128, 2, %[mb]\n\t"
#define ZW4_G2_1                                                                                   \
    "v_lshl_add_u32 v129, v128, 2, %[mb]\n\t"                                                      \
    "v_bfi_b32 v125, %[rmask], %[rp], %[rb]\n\t"

// commit, window n+1's read, the commit mask and y' candidates
#define ZW4_CMT_0(A, N, C, SEL)                                                                    \
    "v_cmp_lt_u32 vcc, %[l], v118\n\t"                                                             \
    "v_add_u32_sdwa " N ", " A ", v118 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0 src1_sel:DWORD\n\t" \
    "s_and_saveexec_b64 s[40:41], vcc\n\t"                                                         \
    "ds_write_b8 " C ", v116\n\t"                                                                  \
    "ds_write_b8 v114, v107\n\t"                                                                   \
    "s_mov_b64 exec, s[40:41]\n\t"                                                                 \
    "ds_read_u8 v107, " N "\n\t"                                                                   \
    "ds_read_u8 v122, v126\n\t"                                                                    \
    "ds_read_b32 v123, v129\n\t"                                                                   \
    "s_and_b64 s[46:47], vcc, s[40:41]\n\t"                                                        \
    SEL
#define ZW4_CMT_1(A, N, C, SEL)                                                                    \
    "v_cmp_lt_u32_e64 s[46:47], %[l], v118\n\t"                                                    \
    "v_add_u32_sdwa " N ", " A ", v118 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0 src1_sel:DWORD\n\t" \
    "s_mov_b64 exec, s[46:47]\n\t"                                                                 \
    "ds_write_b8 " C ", v116\n\t"                                                                  \
    "ds_write_b8 v114, v107\n\t"                                                                   \
    "s_mov_b64 exec, -1\n\t"                                                                       \
    "ds_read_u8 v107, " N "\n\t"                                                                   \
    "ds_read_u8 v122, v126\n\t"                                                                    \
    "ds_read_b32 v123, v129\n\t"                                                                   \
    "v_cndmask_b32_e64 v120, %[y], v130, s[46:47]\n\t"
#define ZW4_SEL_0 "v_cndmask_b32 v120, %[y], v130, vcc\n\t"
#define ZW4_SEL_1                                                                                  \
    "v_cndmask_b32_sdwa v120, v120, v130, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD\n\t"

#define ZW4_XA_0                                                                                   \
    "v_add_u32 %[xa], %[xa], v118\n\t"                                                             \
    "v_and_b32 %[xa], 0xff, %[xa]\n\t"
#define ZW4_XA_1                                                                                   \
    "v_add_u32_sdwa %[xa], %[xa], v118 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"

#define ZW4_WINDOW(A, N, C, G, X, K, Y)                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    "v_add_u32_dpp v112, v107, v107 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"         \
    "v_max_u32_dpp v120, v120, v120 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"            \
    "v_cmp_ge_u32_e64 s[42:43], v123, %[v]\n\t"                                                    \
    "v_add_u32_dpp v112, v112, v112 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_max_u32_dpp v120, v120, v120 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"            \
    "v_add_u32 %[v], 0x100, %[v]\n\t"                                                              \
    "v_add_u32_dpp v112, v112, v112 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_max_u32_dpp v120, v120, v120 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                \
    "s_or_b64 s[42:43], s[42:43], s[44:45]\n\t"                                                    \
    "v_cndmask_b32_e64 v124, v121, v122, s[42:43]\n\t"                                             \
    "v_add_u32_dpp v112, v112, v112 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_max_u32_dpp v120, v120, v120 row_mirror row_mask:0xf bank_mask:0xf\n\t"                     \
    ZW4_JK_##K(Y)                                                                                  \
    "v_lshl_add_u32 v115, v112, 2, %[mb]\n\t"                                                      \
    "ds_read_u8 v116, v114\n\t"                                                                    \
    "ds_max_u32 v115, %[v]\n\t"                                                                    \
    "ds_read_b32 v117, v115\n\t"                                                                   \
    ZW4_RING_##X                                                                                   \
    ZW4_D_##K(Y)                                                                                   \
    "s_waitcnt lgkmcnt(1)\n\t"                                                                     \
    "v_cmp_ne_u32 vcc, v117, %[v]\n\t"                                                             \
    "v_cndmask_b32 v118, v118, v119, vcc\n\t"                                                      \
    "v_add_u32_sdwa v126, v107, v116 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t" \
    ZW4_T_##K                                                                                      \
    "ds_read_u8 v121, v126\n\t"                                                                    \
    "v_or_b32_dpp v118, v118, v118 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"             \
    ZW4_G1_##K                                                                                     \
    "v_or_b32_dpp v118, v118, v118 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"             \
    ZW4_G2_##K                                                                                     \
    "v_or_b32_dpp v118, v118, v118 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                 \
    "v_cmp_le_u32_e64 s[44:45], v119, %[l]\n\t"                                                    \
    G                                                                                              \
    "v_or_b32_dpp v118, v118, v118 row_mirror row_mask:0xf bank_mask:0xf\n\t"                      \
    "v_ffbl_b32 v118, v118\n\t"                                                                    \
    ZW4_CMT_##X(A, N, C, ZW4_SEL_##Y)                                                              \
    ZW4_XA_##K                                                                                     \
    "v_sub_u32 %[rem], %[rem], v118\n\t"                                                           \
    "v_add_u32 %[rp], %[rp], v118\n\t"                                                             \
    "v_cmp_ne_u32 vcc, 0, %[rem]\n\t"

#define ZW4_PRE                                                                                    \
    "s_mov_b64 s[46:47], 0\n\t"                                                                    \
    "v_and_b32 v120, 0xff, %[y]\n\t"                                                               \
    "s_mov_b64 s[44:45], 0\n\t"                                                                    \
    "v_mov_b32 v123, 0\n\t"                                                                        \
    "v_mov_b32 v106, %[sb]\n\t"                                                                    \
    "v_mov_b32 v131, %[sb]\n\t"                                                                    \
    "v_mov_b32 v126, %[sb]\n\t"                                                                    \
    ZW_ADDR("%[xa]")                                                                               \
    "ds_read_u8 v107, v106\n\t"

#define ZW4_DRAIN(X)                                                                               \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                     \
    "v_max_u32_dpp v120, v120, v120 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"            \
    "v_cmp_ge_u32_e64 s[42:43], v123, %[v]\n\t"                                                    \
    "s_or_b64 s[42:43], s[42:43], s[44:45]\n\t"                                                    \
    "v_cndmask_b32_e64 v124, v121, v122, s[42:43]\n\t"                                             \
    "v_max_u32_dpp v120, v120, v120 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"            \
    "s_nop 1\n\t"                                                                                  \
    "v_max_u32_dpp v120, v120, v120 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"                \
    "s_nop 1\n\t"                                                                                  \
    "v_max_u32_dpp v120, v120, v120 row_mirror row_mask:0xf bank_mask:0xf\n\t"                     \
    ZW4_RING_##X                                                                                   \
    "v_and_b32 %[y], 0xff, v120\n\t"                                                               \
    "s_waitcnt lgkmcnt(0)\n\t"

#define ZW4_COPY "v_mov_b32 v131, v106\n\t"
#define ZW4_NOP "s_nop 0\n\t"

// one window per trip
#define ZW4_LOOP1(X, K, Y)                                                                         \
    ZW4_PRE                                                                                        \
    "ZW_LOOP_%=:\n\t"                                                                              \
    ZW4_WINDOW("v106", "v106", "v131", ZW4_COPY, X, K, Y)                                          \
    "s_cbranch_vccnz ZW_LOOP_%=\n\t"                                                               \
    ZW4_DRAIN(X)
// two windows per trip
#define ZW4_LOOP2(X, K, Y)                                                                         \
    ZW4_PRE                                                                                        \
    "ZW_LOOP_%=:\n\t"                                                                              \
    ZW4_WINDOW("v106", "v131", "v106", ZW4_NOP, X, K, Y)                                           \
    "s_cbranch_vccz ZW_DRAIN_%=\n\t"                                                               \
    ZW4_WINDOW("v131", "v106", "v131", ZW4_NOP, X, K, Y)                                           \
    "s_cbranch_vccnz ZW_LOOP_%=\n\t"                                                               \
    "ZW_DRAIN_%=:\n\t"                                                                             \
    ZW4_DRAIN(X)

#define ZW4_OPERANDS                                                                               \
    : [xa] "+v"(w.xa), [y] "+v"(w.y), [v] "+v"(w.v), [rem] "+v"(rem), [rp] "+v"(w.rp)              \
    : [l] "v"(l), [sb] "v"(sb), [mb] "v"(mb), [rb] "v"(rb), [bitl] "v"(bitl), [l1] "v"(l1),        \
      [rmask] "s"(kWinRing - 1)                                                                    \
    : "memory", "vcc", "scc", "v106", "v107", "v112", "v114", "v115", "v116", "v117", "v118", "v119", "v120", \
      "v121", "v122", "v123", "v124", "v125", "v126", "v128", "v129", "v130", "v131", "s40", "s41", \
      "s42", "s43", "s44", "s45", "s46", "s47"

// MODE: 20 X, 21 U, 22 K (+ the y fold), 23 U+X, 24 U+X+K (shipped: mode 6 runs the same loop since),
// 25 X+K, 26 U+K (+ the y fold), 27 none of them: the product loop as it was before U+X+K shipped
template <int MODE>
__device__ __forceinline__ void win_windows_v4(WinLane &w, uint32_t rem, uint32_t l, uint32_t sb, uint32_t mb,
                                               uint32_t rb)
{
    const uint32_t bitl = 1u << l, l1 = (l + 1) << 8;
    if constexpr (MODE == 20) asm volatile(ZW4_LOOP1(1, 0, 0) ZW4_OPERANDS);
    else if constexpr (MODE == 21) asm volatile(ZW4_LOOP2(0, 0, 0) ZW4_OPERANDS);
    else if constexpr (MODE == 22) asm volatile(ZW4_LOOP1(0, 1, 1) ZW4_OPERANDS);
    else if constexpr (MODE == 23) asm volatile(ZW4_LOOP2(1, 0, 0) ZW4_OPERANDS);
    else if constexpr (MODE == 24) asm volatile(ZW4_LOOP2(1, 1, 0) ZW4_OPERANDS);
    else if constexpr (MODE == 25) asm volatile(ZW4_LOOP1(1, 1, 0) ZW4_OPERANDS);
    else if constexpr (MODE == 26) asm volatile(ZW4_LOOP2(0, 1, 1) ZW4_OPERANDS);
    else asm volatile(ZW4_LOOP1(0, 0, 0) ZW4_OPERANDS);
}

}  // namespace zrc4
