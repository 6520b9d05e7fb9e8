// zrc4.hip -- C-ABI implementation (include/zrc4.h) over the gfx950 kernels.
//
// Host side of the drop-in for RC4Encryption (depends/rc4/rc4_encryption.h:43-99).
// The device arena replaces the by-value RC4Encryption members of TcpSession
// (include/zsummerX/frame/session.h:115-116); see INTEGRATION.md.
#include "zrc4.h"
#include "zrc4_plan.hpp"
#include "zrc4_kernels.hpp"
#include "zrc4_win.hpp"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <new>
#include <type_traits>
#include <thread>

struct zrc4_ctx {
    int device;
    int num_cus;
    uint32_t capacity;      // multiple of 256
    uint8_t *arena;         // capacity/256 groups x 64 KiB S-box images
    uint16_t *xy;           // per slot: x | y << 8
    uint8_t *sink;          // crypt_kernel's per-thread sink slots (loads/stores past a
                            // session's last block in the DPP line loop)
    uint32_t *err;          // latched device-side faults (zrc4::kErrWords words, one per
                            // kind) in pinned host memory: kernels latch with a plain
                            // store, the host reads them after the stream wait (no
                            // read-back copy).  Per context, not per stream.
    // staging for the *_host entry points (grown on demand)
    uint8_t *d_stage;
    size_t d_stage_bytes;
    uint8_t *h_stage;       // pinned
    size_t h_stage_bytes;
    hipStream_t stream;     // private stream for the host entry points
    unsigned long long *claim;   // grouped launches' (group, part) claim words (zrc4::Claim), zeroed
    uint32_t epoch;              // the last grouped launch's claim tag
    // Declared bucket groups of large declared launches (decl_check_kernel
    // reads them zero-copy): a ring of coherent pinned buffers, each reused
    // once the check kernel that read it has run (its event).  A pageable
    // hipMemcpyAsync here blocked the host until the stream drained: +4.7 us
    // per cfg3 call back to back (profiles/r05/ab_ids_modes.log).
    static constexpr int kDeclRing = 4;
    uint32_t *h_decl[kDeclRing];
    uint32_t h_decl_cap[kDeclRing];
    hipEvent_t decl_ev[kDeclRing];
    bool decl_ev_live[kDeclRing];
    uint32_t decl_next;
    // zrc4_copy_states' record scratch (n * 258 bytes: S-boxes, then x/y words),
    // owned by the destination context; grown on demand and kept
    uint8_t *copy_scratch;
    size_t copy_scratch_bytes;
    // the last copy's end: a copy on another stream waits for it before it
    // reuses the scratch
    hipEvent_t copy_ev;
    hipStream_t copy_last;
    bool copy_ev_live;
};

namespace {

int hip_err(hipError_t e) { return e == hipSuccess ? ZRC4_OK : ZRC4_ERR_HIP; }

#define ZRC4_TRY(expr)                          \
    do {                                        \
        hipError_t e_ = (expr);                 \
        if (e_ != hipSuccess) return ZRC4_ERR_HIP; \
    } while (0)

int set_device(const zrc4_ctx *c)
{
    return hip_err(hipSetDevice(c->device));
}

int grow_stage(zrc4_ctx *c, size_t bytes)
{
    if (bytes <= c->d_stage_bytes && bytes <= c->h_stage_bytes) return ZRC4_OK;
    size_t want = 1u << 20;
    while (want < bytes) want <<= 1;
    if (c->d_stage) (void)hipFree(c->d_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    c->d_stage = nullptr;
    c->h_stage = nullptr;
    c->d_stage_bytes = c->h_stage_bytes = 0;
    if (hipMalloc(&c->d_stage, want) != hipSuccess) return ZRC4_ERR_OUT_OF_MEMORY;
    // coherent: small batches run on it in place, and kernels are dispatched
    // with agent-scope acquire (a non-coherent line could be stale in L2)
    if (hipHostMalloc(&c->h_stage, want, hipHostMallocCoherent) != hipSuccess)
        return ZRC4_ERR_OUT_OF_MEMORY;
    c->d_stage_bytes = c->h_stage_bytes = want;
    return ZRC4_OK;
}

size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

constexpr size_t kZeroCopyMax = 256u << 10;   // *_host batches up to this size run on pinned staging in place

int launched() { return hipGetLastError() == hipSuccess ? ZRC4_OK : ZRC4_ERR_LAUNCH; }

// One crypt, keystream or out-of-place call, as launch_crypt takes it.
struct CryptCall {
    int mode = zrc4::kRange;            // zrc4::CryptMode
    const uint32_t *ids = nullptr;
    uint32_t first_slot = 0;
    uint8_t *payload = nullptr;         // kIoKs / kIoTo / kIoToRounds: the destination
    const uint64_t *off = nullptr;
    const uint32_t *len = nullptr;
    uint32_t n = 0;
    const zrc4::FrameArgs *frame = nullptr;   // the framing walk of every entry runs in the same launch
    const uint32_t *decl = nullptr;     // kGrouped: the declared group per 256-entry bucket, in host memory
    bool trusted = false;               // ... computed here from host ids (zrc4_crypt_host, the reservoirs)
    int io = zrc4::kIoInPlace;          // zrc4::CryptIo
    const uint8_t *src = nullptr;       // kIoTo / kIoToRounds: entry i reads src + src_off[i]
    const uint64_t *src_off = nullptr;
    uint32_t rounds = 1;                // kIoToRounds: off, len and src_off hold rounds * n entries, round-major
};

// The arguments every call has, in the public entry points' order; a caller
// sets the others by name.
CryptCall crypt_call(int mode, const uint32_t *ids, uint32_t first_slot, uint8_t *payload, const uint64_t *off,
                     const uint32_t *len, uint32_t n)
{
    CryptCall k;
    k.mode = mode;
    k.ids = ids;
    k.first_slot = first_slot;
    k.payload = payload;
    k.off = off;
    k.len = len;
    k.n = n;
    return k;
}

// A runtime value out of a closed list, and with_constants: f(constants...)
// with every value replaced by the std::integral_constant it equals (f is not
// called if one of them is outside its list).
template <typename T, T... Vs>
struct OneOf {
    T v;
};
using ModeOf = OneOf<int, zrc4::kIds, zrc4::kRange, zrc4::kGrouped>;
using IoOf = OneOf<int, zrc4::kIoInPlace, zrc4::kIoKs, zrc4::kIoTo, zrc4::kIoToRounds>;
using BoolOf = OneOf<bool, false, true>;

template <typename F>
void with_constants(F &&f)
{
    f();
}
template <typename F, typename T, T... Vs, typename... Rest>
void with_constants(F &&f, OneOf<T, Vs...> head, Rest... rest)
{
    (void)((head.v == Vs &&
            (with_constants([&](auto... cs) { f(std::integral_constant<T, Vs>{}, cs...); }, rest...), true)) ||
           ...);
}

// What a kernel of form IO takes in its FrameArgs position.
template <int IO>
zrc4::AuxArgs<IO> aux_args(const CryptCall &k)
{
    if constexpr (std::is_same_v<zrc4::AuxArgs<IO>, zrc4::ToArgs>) {
        zrc4::ToArgs ta{};
        ta.src = k.src;
        ta.src_off = k.src_off;
        ta.rounds = k.rounds;
        ta.stride = k.n;
        return ta;
    } else {
        return k.frame ? *k.frame : zrc4::FrameArgs{};
    }
}

// The five kernel families, one launch site each.  A launch exists only for
// the forms zrc4_plan.hpp's predicates name; a plan outside them (there is
// none) is ZRC4_ERR_INTERNAL.
int launch_win(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, const zrc4::Claim &cl, hipStream_t s)
{
    zrc4::WinGroups dg{};
    if (p.decl)
        for (uint32_t b = 0; b < p.groups; ++b) dg.g[b] = k.decl[b];
    bool hit = false;
    with_constants(
        [&](auto M, auto F, auto D, auto IO) {
            if constexpr (zrc4::win_form_exists(M, F, D, IO)) {
                hipLaunchKernelGGL((zrc4::crypt_win_kernel<M, F, D, IO>), dim3(p.grid), dim3(p.block), 0, s, c->arena,
                                   c->xy, k.ids, k.first_slot, k.payload, k.off, k.len, k.n, c->capacity, c->err,
                                   c->sink, aux_args<IO>(k), cl, dg);
                hit = true;
            }
        },
        ModeOf{p.mode}, BoolOf{p.frame}, BoolOf{p.decl}, IoOf{p.io});
    return hit ? launched() : ZRC4_ERR_INTERNAL;
}

int launch_decl(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, const zrc4::Claim &cl, hipStream_t s)
{
    zrc4::BucketGroups dg{};
    for (uint32_t b = 0; b < p.groups; ++b) dg.g[b] = k.decl[b];
    bool hit = false;
    with_constants(
        [&](auto F, auto H, auto IO) {
            if constexpr (zrc4::decl_form_exists(F, H, IO)) {
                hipLaunchKernelGGL((zrc4::crypt_decl_kernel<F, H, IO>), dim3(p.grid), dim3(p.block), 0, s, c->arena,
                                   c->xy, k.ids, k.payload, k.off, k.len, k.n, c->capacity, c->err, c->sink,
                                   aux_args<IO>(k), cl, dg);
                hit = true;
            }
        },
        BoolOf{p.frame}, BoolOf{p.half}, IoOf{p.io});
    return hit ? launched() : ZRC4_ERR_INTERNAL;
}

int launch_half(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, const zrc4::Claim &cl, hipStream_t s)
{
    bool hit = false;
    with_constants(
        [&](auto M, auto F, auto IO) {
            if constexpr (zrc4::half_form_exists(M, F, IO)) {
                hipLaunchKernelGGL((zrc4::crypt_half_kernel<M, F, IO>), dim3(p.grid), dim3(p.block), 0, s, c->arena,
                                   c->xy, k.ids, k.first_slot, k.payload, k.off, k.len, k.n, c->capacity, c->err,
                                   c->sink, aux_args<IO>(k), cl);
                hit = true;
            }
        },
        ModeOf{p.mode}, BoolOf{p.frame}, IoOf{p.io});
    return hit ? launched() : ZRC4_ERR_INTERNAL;
}

int launch_whole(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, const zrc4::Claim &cl, hipStream_t s)
{
    bool hit = false;
    with_constants(
        [&](auto M, auto F, auto IO) {
            if constexpr (zrc4::whole_form_exists(M, F, IO)) {
                hipLaunchKernelGGL((zrc4::crypt_kernel<M, F, IO>), dim3(p.grid), dim3(p.block), 0, s, c->arena, c->xy,
                                   k.ids, k.first_slot, k.payload, k.off, k.len, k.n, c->capacity, c->err, c->sink,
                                   aux_args<IO>(k), cl);
                hit = true;
            }
        },
        ModeOf{p.mode}, BoolOf{p.frame}, IoOf{p.io});
    return hit ? launched() : ZRC4_ERR_INTERNAL;
}

int launch_stream(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, const zrc4::Claim &cl, hipStream_t s)
{
    bool hit = false;
    with_constants(
        [&](auto PF, auto GR, auto F) {
            if constexpr (zrc4::stream_form_exists(PF, GR, F)) {
                hipLaunchKernelGGL((zrc4::crypt_stream_kernel<PF, GR, F>), dim3(p.grid), dim3(p.block), 0, s,
                                   c->arena, c->xy, k.ids, k.first_slot, k.payload, k.off, k.len, k.n, c->capacity,
                                   c->err, c->sink, cl, aux_args<zrc4::kIoInPlace>(k));
                hit = true;
            }
        },
        BoolOf{p.pf}, BoolOf{p.gr}, BoolOf{p.frame});
    return hit ? launched() : ZRC4_ERR_INTERNAL;
}

// A fresh claim tag per grouped launch; on the 32-bit wrap the words are
// zeroed first (stream-ordered before this launch).
int next_claim(zrc4_ctx *c, hipStream_t s, zrc4::Claim &cl)
{
    const size_t words = (size_t)(c->capacity / zrc4::kGroup) * zrc4::kClaimParts;
    if (++c->epoch == 0u) {
        ZRC4_TRY(hipMemsetAsync(c->claim, 0, words * 8u, s));
        c->epoch = 1u;
    }
    cl = zrc4::Claim{c->claim, c->epoch, reinterpret_cast<const uint32_t *>(c->claim + words)};
    return ZRC4_OK;
}

// Check the declared groups before the crypt launch (stream-ordered): a
// disagreeing bucket's groups are claimed under this launch's epoch.  The
// groups go through the context's ring of pinned buffers (zrc4_ctx::h_decl).
int check_declared(zrc4_ctx *c, const CryptCall &k, uint32_t buckets, const zrc4::Claim &cl, hipStream_t s)
{
    const int r = (int)(c->decl_next++ % (uint32_t)zrc4_ctx::kDeclRing);
    if (c->decl_ev_live[r]) ZRC4_TRY(hipEventSynchronize(c->decl_ev[r]));    // its last reader has run
    if (!c->decl_ev[r] && hipEventCreateWithFlags(&c->decl_ev[r], hipEventDisableTiming) != hipSuccess)
        return ZRC4_ERR_HIP;
    if (buckets > c->h_decl_cap[r]) {
        if (c->h_decl[r]) (void)hipHostFree(c->h_decl[r]);
        c->h_decl[r] = nullptr;
        c->h_decl_cap[r] = 0;
        uint32_t want = 1024u;
        while (want < buckets) want <<= 1;
        void *p = nullptr;
        if (hipHostMalloc(&p, (size_t)want * 4u, hipHostMallocCoherent) != hipSuccess) return ZRC4_ERR_OUT_OF_MEMORY;
        c->h_decl[r] = static_cast<uint32_t *>(p);
        c->h_decl_cap[r] = want;
    }
    memcpy(c->h_decl[r], k.decl, (size_t)buckets * 4u);
    hipLaunchKernelGGL(zrc4::decl_check_kernel, dim3(buckets), dim3(zrc4::kGroup), 0, s, k.ids, k.len, k.n,
                       c->h_decl[r], c->capacity, cl, c->err);
    if (int rc = launched()) return rc;
    ZRC4_TRY(hipEventRecord(c->decl_ev[r], s));
    c->decl_ev_live[r] = true;
    return ZRC4_OK;
}

// One planned launch: the claim epoch (grouped), the up-front check and the
// pre-kernel the plan asks for, then the kernel.
int issue_crypt(zrc4_ctx *c, const CryptCall &k, const zrc4::CryptPlan &p, hipStream_t s)
{
    int rc = ZRC4_OK;
    zrc4::Claim cl{nullptr, 0u, nullptr};
    if (k.mode == zrc4::kGrouped && (rc = next_claim(c, s, cl))) return rc;
    if (p.check && (rc = check_declared(c, k, p.groups, cl, s))) return rc;
    const uint32_t *span_ids = k.mode == zrc4::kGrouped ? k.ids : nullptr;
    if (p.pre == zrc4::kPreFill)
        hipLaunchKernelGGL(zrc4::span_fill_kernel, dim3(p.pre_grid), dim3(zrc4::kGroup), 0, s, span_ids, k.payload,
                           k.off, k.len, k.n, c->capacity);
    if (p.pre == zrc4::kPreCopy)
        hipLaunchKernelGGL(zrc4::span_copy_kernel, dim3(p.pre_grid), dim3(zrc4::kGroup), 0, s, span_ids, k.src,
                           k.src_off, k.payload, k.off, k.len, k.n, c->capacity);
    if (p.pre != zrc4::kPreNone && (rc = launched())) return rc;
    switch (p.family) {
    case zrc4::kFamWin: return launch_win(c, k, p, cl, s);
    case zrc4::kFamDecl: return launch_decl(c, k, p, cl, s);
    case zrc4::kFamHalf: return launch_half(c, k, p, cl, s);
    case zrc4::kFamWhole: return launch_whole(c, k, p, cl, s);
    case zrc4::kFamStream: return launch_stream(c, k, p, cl, s);
    }
    return ZRC4_ERR_INTERNAL;
}

// Every crypt, keystream and out-of-place call: validate, plan (plan_crypt,
// zrc4_plan.hpp: the rules and their measured reasons), then the plan's side
// effects and its kernel (issue_crypt) -- once, or once per round where the
// plan splits a rounds call into kIoTo calls on the stream.
int launch_crypt(zrc4_ctx *c, const CryptCall &k, hipStream_t s)
{
    if (k.n == 0) return ZRC4_OK;
    const bool out_of_place = k.io == zrc4::kIoTo || k.io == zrc4::kIoToRounds;
    if (out_of_place && (!k.src || !k.src_off)) return ZRC4_ERR_INVALID_ARG;
    zrc4::CryptShape sh{};
    sh.mode = k.mode;
    sh.first_aligned = (k.first_slot & 255u) == 0u;
    sh.n = k.n;
    sh.rounds = k.rounds;
    sh.cus = (uint32_t)c->num_cus;
    sh.frame = k.frame != nullptr;
    sh.declared = k.decl != nullptr;
    sh.trusted = k.trusted;
    sh.io = k.io;
    const zrc4::CryptPlan p = zrc4::plan_crypt(sh);
    if (p.err != zrc4::kPlanOk) return ZRC4_ERR_INVALID_ARG;
    if (k.mode == zrc4::kRange && (uint64_t)k.first_slot + k.n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
    if (!p.split) return issue_crypt(c, k, p, s);
    CryptCall one = k;
    one.io = zrc4::kIoTo;
    one.rounds = 1;
    for (uint32_t r = 0; r < k.rounds; ++r) {
        const size_t at = (size_t)r * k.n;
        one.off = k.off + at;
        one.len = k.len + at;
        one.src_off = k.src_off + at;
        if (int rc = issue_crypt(c, one, p, s)) return rc;
    }
    return ZRC4_OK;
}

int launch_ksa(zrc4_ctx *c, const uint32_t *ids, uint32_t first_slot, const uint8_t *keys,
               const uint64_t *key_off, const uint32_t *key_len, uint32_t n, hipStream_t s)
{
    if (n == 0) return ZRC4_OK;
    if (!ids && (uint64_t)first_slot + n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
    const uint32_t grid = (n + zrc4::kGroup - 1) / zrc4::kGroup;
    hipLaunchKernelGGL(zrc4::ksa_kernel, dim3(grid), dim3(zrc4::kGroup), 0, s, c->arena, c->xy,
                       ids, first_slot, keys, key_off, key_len, n, c->capacity, c->err);
    return launched();
}

// Record export / import (zrc4_export_states and friends; kernels and paths:
// zrc4_kernels.hpp).  Records move as 16-byte pieces, so sbox must be 16-byte
// aligned.  gate / gate_cap: zrc4_copy_states' source ids, so that an entry
// whose source was skipped is skipped on the import side too.
bool records_ok(const void *sbox, const void *xy)
{
    return sbox && xy && ((uintptr_t)sbox & 15u) == 0u && ((uintptr_t)xy & 1u) == 0u;
}

uint32_t range_groups(uint32_t first_slot, uint32_t n)
{
    return ((first_slot + (n - 1u)) >> 8) - (first_slot >> 8) + 1u;
}

int launch_export(zrc4_ctx *c, const uint32_t *ids, uint32_t first_slot, uint32_t n, uint8_t *sbox, uint16_t *xy,
                  hipStream_t s)
{
    if (n == 0) return ZRC4_OK;
    if (!records_ok(sbox, xy)) return ZRC4_ERR_INVALID_ARG;
    if (!ids) {
        if ((uint64_t)first_slot + n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
        hipLaunchKernelGGL(zrc4::states_export_kernel<true>, dim3(range_groups(first_slot, n)), dim3(zrc4::kGroup), 0,
                           s, c->arena, c->xy, ids, first_slot, n, c->capacity, sbox, xy, c->err);
    } else {
        const uint32_t buckets = (uint32_t)(((uint64_t)n + zrc4::kGroup - 1) / zrc4::kGroup);
        hipLaunchKernelGGL(zrc4::states_export_kernel<false>, dim3(buckets), dim3(zrc4::kGroup), 0, s, c->arena,
                           c->xy, ids, 0u, n, c->capacity, sbox, xy, c->err);
    }
    return launched();
}

int launch_import(zrc4_ctx *c, const uint32_t *ids, uint32_t first_slot, uint32_t n, const uint8_t *sbox,
                  const uint16_t *xy, const uint32_t *gate, uint32_t gate_cap, hipStream_t s)
{
    if (n == 0) return ZRC4_OK;
    if (!records_ok(sbox, xy)) return ZRC4_ERR_INVALID_ARG;
    if (!ids) {
        if ((uint64_t)first_slot + n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
        hipLaunchKernelGGL(zrc4::states_import_image_kernel, dim3(range_groups(first_slot, n)), dim3(zrc4::kGroup), 0,
                           s, c->arena, c->xy, first_slot, n, sbox, xy, gate, gate_cap);
    } else {
        const uint32_t grid = (uint32_t)(((uint64_t)n + 3u) / 4u);
        hipLaunchKernelGGL(zrc4::states_scatter_kernel, dim3(grid), dim3(256), 0, s, c->arena, c->xy, ids, n,
                           c->capacity, sbox, xy, gate, gate_cap, c->err);
    }
    return launched();
}

// The per-iteration completion point of the session engine's hooks: ONE
// stream wait, then the latch word is read straight from pinned memory (a
// device-to-host copy of it used to cost another ~11 us per call).
int read_faults(zrc4_ctx *c)
{
    volatile uint32_t *e = c->err;
    int rc = ZRC4_OK;
    if (e[zrc4::kErrLdsLayout]) rc = ZRC4_ERR_INTERNAL;
    else if (e[zrc4::kErrGroup]) rc = ZRC4_ERR_GROUP;
    else if (e[zrc4::kErrSlotRange]) rc = ZRC4_ERR_SLOT_RANGE;
    for (uint32_t i = 0; i < zrc4::kErrWords; ++i) e[i] = 0u;
    return rc;
}

int check_err(zrc4_ctx *c, hipStream_t s)
{
    ZRC4_TRY(hipStreamSynchronize(s));
    return read_faults(c);
}

}  // namespace

extern "C" {

int zrc4_create(zrc4_ctx **out, int device, uint32_t capacity)
{
    if (!out || capacity == 0) return ZRC4_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ZRC4_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return ZRC4_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ZRC4_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ZRC4_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ZRC4_ERR_NO_DEVICE;

    zrc4_ctx *c = new (std::nothrow) zrc4_ctx();
    if (!c) return ZRC4_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    const uint64_t cap = ((uint64_t)capacity + 255u) & ~(uint64_t)255u;
    if (cap > 0xFFFFFF00ull) { delete c; return ZRC4_ERR_INVALID_ARG; }
    c->capacity = (uint32_t)cap;
    const size_t groups = c->capacity / zrc4::kGroup;
    bool ok = hipMalloc(&c->arena, groups * (size_t)zrc4::kGroupBytes) == hipSuccess &&
              hipMalloc(&c->xy, (size_t)c->capacity * sizeof(uint16_t)) == hipSuccess &&
              hipMalloc(&c->sink, zrc4::kSinkBytes) == hipSuccess &&
              hipHostMalloc(&c->err, zrc4::kErrWords * sizeof(uint32_t), hipHostMallocCoherent) == hipSuccess &&
              // + 16 zero bytes after the claim words (Claim::zero; the epoch-wrap memset stops before them)
              hipMalloc(&c->claim, (groups * zrc4::kClaimParts + 2) * sizeof(unsigned long long)) == hipSuccess &&
              hipMemset(c->claim, 0, (groups * zrc4::kClaimParts + 2) * sizeof(unsigned long long)) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    if (!ok) { zrc4_destroy(c); return ZRC4_ERR_OUT_OF_MEMORY; }
    // Fresh slots hold the reference's empty-key state: identity box, x = y = 0
    // (what makeSBox("") produces, rc4_encryption.h:48-53).
    for (uint32_t i = 0; i < zrc4::kErrWords; ++i) c->err[i] = 0u;
    hipLaunchKernelGGL(zrc4::identity_kernel, dim3((unsigned)groups), dim3(zrc4::kGroup), 0,
                       c->stream, c->arena);
    if (hipGetLastError() != hipSuccess ||
        hipMemsetAsync(c->xy, 0, (size_t)c->capacity * sizeof(uint16_t), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        zrc4_destroy(c);
        return ZRC4_ERR_HIP;
    }
    *out = c;
    return ZRC4_OK;
}

int zrc4_destroy(zrc4_ctx *c)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->xy) (void)hipFree(c->xy);
    if (c->sink) (void)hipFree(c->sink);
    if (c->claim) (void)hipFree(c->claim);
    for (int k = 0; k < zrc4_ctx::kDeclRing; ++k) {
        if (c->decl_ev_live[k]) (void)hipEventSynchronize(c->decl_ev[k]);   // a check kernel may still read h_decl
        if (c->decl_ev[k]) (void)hipEventDestroy(c->decl_ev[k]);
        if (c->h_decl[k]) (void)hipHostFree(c->h_decl[k]);
    }
    if (c->err) (void)hipHostFree(c->err);
    if (c->d_stage) (void)hipFree(c->d_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->copy_scratch) (void)hipFree(c->copy_scratch);
    if (c->copy_ev) (void)hipEventDestroy(c->copy_ev);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return ZRC4_OK;
}

uint32_t zrc4_capacity(const zrc4_ctx *c) { return c ? c->capacity : 0u; }

int zrc4_ksa(zrc4_ctx *c, const uint32_t *ids, const uint8_t *keys, const uint64_t *key_off,
             const uint32_t *key_len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!key_len || !key_off)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_ksa(c, ids, 0, keys, key_off, key_len, n, (hipStream_t)stream);
}

int zrc4_crypt(zrc4_ctx *c, const uint32_t *ids, uint8_t *payload, const uint64_t *off,
               const uint32_t *len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_crypt(c, crypt_call(ids ? zrc4::kIds : zrc4::kRange, ids, 0, payload, off, len, n),
                        (hipStream_t)stream);
}

int zrc4_ksa_range(zrc4_ctx *c, uint32_t first_slot, const uint8_t *keys,
                   const uint64_t *key_off, const uint32_t *key_len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!key_len || !key_off)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_ksa(c, nullptr, first_slot, keys, key_off, key_len, n, (hipStream_t)stream);
}

int zrc4_crypt_range(zrc4_ctx *c, uint32_t first_slot, uint8_t *payload, const uint64_t *off,
                     const uint32_t *len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_crypt(c, crypt_call(zrc4::kRange, nullptr, first_slot, payload, off, len, n), (hipStream_t)stream);
}

int zrc4_crypt_grouped(zrc4_ctx *c, const uint32_t *ids, uint8_t *payload, const uint64_t *off,
                       const uint32_t *len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!ids || !payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_crypt(c, crypt_call(zrc4::kGrouped, ids, 0, payload, off, len, n), (hipStream_t)stream);
}

namespace {
// A call's declared bucket groups (none declared: fine): each names a group of
// the arena, or ZRC4_IDLE_SLOT for a bucket with no busy entry.
bool bucket_groups_ok(const zrc4_ctx *c, const uint32_t *bucket_group, uint32_t n)
{
    if (!bucket_group) return true;
    const uint32_t nb = (uint32_t)(((uint64_t)n + zrc4::kGroup - 1) / zrc4::kGroup);
    const uint32_t groups = c->capacity / zrc4::kGroup;
    for (uint32_t b = 0; b < nb; ++b)
        if (bucket_group[b] >= groups && bucket_group[b] != ZRC4_IDLE_SLOT) return false;
    return true;
}

int frame_args(const zrc4_frame_args *f, uint32_t n, zrc4::FrameArgs &out)
{
    if (!f) return ZRC4_ERR_INVALID_ARG;
    if (n && (!f->off || !f->len || !f->npk || !f->used || !f->status || (f->max_packets && !f->pkt_len)))
        return ZRC4_ERR_INVALID_ARG;
    out.off = f->off;
    out.len = f->len;
    out.bound = f->bound;
    out.maxp = f->max_packets;
    out.npk = f->npk;
    out.used = f->used;
    out.status = f->status;
    out.pkt_len = f->max_packets ? f->pkt_len : nullptr;
    return ZRC4_OK;
}
}  // namespace

int zrc4_crypt_range_frame(zrc4_ctx *c, uint32_t first_slot, uint8_t *payload, const uint64_t *off,
                           const uint32_t *len, uint32_t n, const zrc4_frame_args *frame, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    zrc4::FrameArgs fr;
    int rc = frame_args(frame, n, fr);
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    CryptCall k = crypt_call(zrc4::kRange, nullptr, first_slot, payload, off, len, n);
    k.frame = &fr;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_grouped_frame(zrc4_ctx *c, const uint32_t *ids, uint8_t *payload, const uint64_t *off,
                             const uint32_t *len, uint32_t n, const zrc4_frame_args *frame, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!ids || !payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    zrc4::FrameArgs fr;
    int rc = frame_args(frame, n, fr);
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    CryptCall k = crypt_call(zrc4::kGrouped, ids, 0, payload, off, len, n);
    k.frame = &fr;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_grouped_declared(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, uint8_t *payload,
                                const uint64_t *off, const uint32_t *len, uint32_t n,
                                const struct zrc4_frame_args *frame, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!ids || !bucket_group || !payload || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    if (!bucket_groups_ok(c, bucket_group, n)) return ZRC4_ERR_INVALID_ARG;
    zrc4::FrameArgs fr;
    int rc = frame ? frame_args(frame, n, fr) : ZRC4_OK;
    if (rc) return rc;
    if ((rc = set_device(c))) return rc;
    CryptCall k = crypt_call(zrc4::kGrouped, ids, 0, payload, off, len, n);
    k.frame = frame ? &fr : nullptr;
    k.decl = bucket_group;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_keystream_range(zrc4_ctx *c, uint32_t first_slot, uint8_t *out, const uint64_t *off, const uint32_t *len,
                         uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!out || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kRange, nullptr, first_slot, out, off, len, n);
    k.io = zrc4::kIoKs;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_keystream_grouped(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, uint8_t *out,
                           const uint64_t *off, const uint32_t *len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!ids || !out || !off || !len)) return ZRC4_ERR_INVALID_ARG;
    if (!bucket_groups_ok(c, bucket_group, n)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kGrouped, ids, 0, out, off, len, n);
    k.decl = bucket_group;
    k.io = zrc4::kIoKs;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_to_range(zrc4_ctx *c, uint32_t first_slot, const uint8_t *src, const uint64_t *src_off, uint8_t *dst,
                        const uint64_t *dst_off, const uint32_t *len, uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!src || !src_off || !dst || !dst_off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kRange, nullptr, first_slot, dst, dst_off, len, n);
    k.io = zrc4::kIoTo;
    k.src = src;
    k.src_off = src_off;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_to_grouped(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, const uint8_t *src,
                          const uint64_t *src_off, uint8_t *dst, const uint64_t *dst_off, const uint32_t *len,
                          uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n && (!ids || !src || !src_off || !dst || !dst_off || !len)) return ZRC4_ERR_INVALID_ARG;
    if (!bucket_groups_ok(c, bucket_group, n)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kGrouped, ids, 0, dst, dst_off, len, n);
    k.decl = bucket_group;
    k.io = zrc4::kIoTo;
    k.src = src;
    k.src_off = src_off;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_to_range_rounds(zrc4_ctx *c, uint32_t first_slot, const uint8_t *src, const uint64_t *src_off,
                               uint8_t *dst, const uint64_t *dst_off, const uint32_t *len, uint32_t n, uint32_t rounds,
                               void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (rounds == 0u || rounds > ZRC4_MAX_ROUNDS || (uint64_t)n * rounds > 0xFFF00000u) return ZRC4_ERR_INVALID_ARG;
    if (rounds == 1u) return zrc4_crypt_to_range(c, first_slot, src, src_off, dst, dst_off, len, n, stream);
    if (n && (!src || !src_off || !dst || !dst_off || !len)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kRange, nullptr, first_slot, dst, dst_off, len, n);
    k.io = zrc4::kIoToRounds;
    k.src = src;
    k.src_off = src_off;
    k.rounds = rounds;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_crypt_to_grouped_rounds(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, const uint8_t *src,
                                 const uint64_t *src_off, uint8_t *dst, const uint64_t *dst_off, const uint32_t *len,
                                 uint32_t n, uint32_t rounds, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (rounds == 0u || rounds > ZRC4_MAX_ROUNDS || (uint64_t)n * rounds > 0xFFF00000u) return ZRC4_ERR_INVALID_ARG;
    if (rounds == 1u) return zrc4_crypt_to_grouped(c, ids, bucket_group, src, src_off, dst, dst_off, len, n, stream);
    if (n && (!ids || !src || !src_off || !dst || !dst_off || !len)) return ZRC4_ERR_INVALID_ARG;
    if (!bucket_groups_ok(c, bucket_group, n)) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    CryptCall k = crypt_call(zrc4::kGrouped, ids, 0, dst, dst_off, len, n);
    k.decl = bucket_group;
    k.io = zrc4::kIoToRounds;
    k.src = src;
    k.src_off = src_off;
    k.rounds = rounds;
    return launch_crypt(c, k, (hipStream_t)stream);
}

int zrc4_xor_ring(zrc4_ctx *c, uint8_t *ring, uint32_t ring_cap, const uint32_t *rid,
                  const uint32_t *pos, uint8_t *payload, const uint64_t *off, const uint32_t *len,
                  uint32_t n, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!ring || ring_cap == 0 || !rid || !pos || !payload || !off || !len) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    hipLaunchKernelGGL(zrc4::xor_ring_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, ring, ring_cap,
                       rid, pos, payload, off, len, n);
    return launched();
}

int zrc4_frame_scan(zrc4_ctx *c, const uint8_t *buf, const uint64_t *off, const uint32_t *len,
                    uint32_t bound, uint32_t n, uint32_t max_packets, uint32_t *npk, uint32_t *used,
                    uint32_t *status, uint32_t *pkt_len, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!buf || !off || !len || !npk || !used || !status || (max_packets && !pkt_len))
        return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    hipLaunchKernelGGL(zrc4::frame_scan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream,
                       buf, off, len, bound, n, max_packets, npk, used, status, max_packets ? pkt_len : nullptr);
    return launched();
}

int zrc4_poll_faults(zrc4_ctx *c)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    return read_faults(c);
}

int zrc4_sync(zrc4_ctx *c, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    return check_err(c, (hipStream_t)stream);
}

int zrc4_ksa_host(zrc4_ctx *c, const uint32_t *ids, const uint8_t *keys, size_t keys_bytes,
                  const uint64_t *key_off, const uint32_t *key_len, uint32_t n)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!key_off || !key_len || (keys_bytes && !keys)) return ZRC4_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (key_len[i] && (key_off[i] > keys_bytes || key_len[i] > keys_bytes - key_off[i]))
            return ZRC4_ERR_INVALID_ARG;
    int rc = set_device(c);
    if (rc) return rc;
    const size_t o_ids = 0, s_ids = ids ? align16((size_t)n * 4) : 0;
    const size_t o_off = o_ids + s_ids, s_off = align16((size_t)n * 8);
    const size_t o_len = o_off + s_off, s_len = align16((size_t)n * 4);
    const size_t o_key = o_len + s_len, total = o_key + align16(keys_bytes ? keys_bytes : 1);
    if ((rc = grow_stage(c, total))) return rc;
    if (ids) memcpy(c->h_stage + o_ids, ids, (size_t)n * 4);
    memcpy(c->h_stage + o_off, key_off, (size_t)n * 8);
    memcpy(c->h_stage + o_len, key_len, (size_t)n * 4);
    if (keys_bytes) memcpy(c->h_stage + o_key, keys, keys_bytes);
    // Small batches run on the pinned staging copy in place (zero-copy over
    // PCIe: one launch and one wait instead of copy + launch + wait).
    uint8_t *st = c->h_stage;
    if (total > kZeroCopyMax) {
        ZRC4_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, total, hipMemcpyHostToDevice, c->stream));
        st = c->d_stage;
    }
    rc = launch_ksa(c, ids ? (const uint32_t *)(st + o_ids) : nullptr, 0,
                    st + o_key, (const uint64_t *)(st + o_off), (const uint32_t *)(st + o_len), n, c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);     // a queued H2D still reads the staging buffer
        return rc;
    }
    return check_err(c, c->stream);
}

// Payload staging copies of the *_host calls (caller memory <-> pinned
// staging): one host thread moves ~8 GB/s, so copies of 2 MiB and more are
// split over up to 8 threads (r06: 512 MiB took ~67 ms on one thread).  If
// a thread cannot be started, its share is copied on the calling thread.
static void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n)
{
    constexpr size_t kPerThreadMin = 1u << 20;
    size_t nt = n / kPerThreadMin;
    const unsigned hw = std::thread::hardware_concurrency();
    if (nt > 8) nt = 8;
    if (hw && nt > hw) nt = hw;
    if (nt <= 1) {
        memcpy(dst, src, n);
        return;
    }
    const size_t per = ((n + nt - 1) / nt + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    size_t started = 1;                     // chunk 0 is this thread's
    try {
        th.reserve(nt - 1);
        for (; started < nt && started * per < n; ++started) {
            const size_t a = started * per, len = std::min(per, n - a);
            th.emplace_back([=] { memcpy(dst + a, src + a, len); });
        }
    } catch (...) {
    }
    memcpy(dst, src, std::min(per, n));
    for (size_t t = started; t * per < n; ++t) memcpy(dst + t * per, src + t * per, std::min(per, n - t * per));
    for (auto &t : th) t.join();
}

// The chunked D2H of a piped zrc4_crypt_host: chunk k's copy is recorded
// with an event and copied out to the caller once it has landed, while the
// later chunks are still in flight.  The kernel ran before the first chunk's
// copy, so the fault latch is final once that chunk has landed: on a fault
// nothing is copied out (as on the unpiped path).  Without events (creation
// failed) it waits for the stream and copies everything at once.
static constexpr size_t kPipeChunk = 16u << 20;

static int copy_back_piped(zrc4_ctx *c, uint8_t *payload, size_t o_pay, size_t payload_bytes)
{
    std::vector<hipEvent_t> ev;
    ev.reserve(payload_bytes / kPipeChunk + 1);
    bool evs = true, copies = true;
    for (size_t a = 0; a < payload_bytes; a += kPipeChunk) {
        const size_t l = std::min(kPipeChunk, payload_bytes - a);
        hipError_t e = hipMemcpyAsync(c->h_stage + o_pay + a, c->d_stage + o_pay + a, l, hipMemcpyDeviceToHost,
                                      c->stream);
        if (e != hipSuccess) copies = evs = false;
        hipEvent_t x = nullptr;
        if (evs && hipEventCreateWithFlags(&x, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(x, c->stream) == hipSuccess) {
                ev.push_back(x);
                continue;
            }
            (void)hipEventDestroy(x);
        }
        evs = false;
    }
    int rc = ZRC4_OK;
    if (!copies) {                         // a chunk never left the device: copy nothing out
        rc = check_err(c, c->stream);
        if (rc == ZRC4_OK) rc = ZRC4_ERR_HIP;
    } else if (!evs || ev.empty() || hipEventSynchronize(ev[0]) != hipSuccess) {
        rc = check_err(c, c->stream);
        if (rc == ZRC4_OK) par_memcpy(payload, c->h_stage + o_pay, payload_bytes);
    } else if ((rc = read_faults(c)) == ZRC4_OK) {
        for (size_t k = 0, a = 0; a < payload_bytes; ++k, a += kPipeChunk) {
            if (hipEventSynchronize(ev[k]) != hipSuccess) {
                rc = ZRC4_ERR_HIP;
                break;
            }
            par_memcpy(payload + a, c->h_stage + o_pay + a, std::min(kPipeChunk, payload_bytes - a));
        }
    }
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t x : ev) (void)hipEventDestroy(x);
    return rc;
}

int zrc4_crypt_host(zrc4_ctx *c, const uint32_t *ids, uint8_t *payload, size_t payload_bytes,
                    const uint64_t *off, const uint32_t *len, uint32_t n)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!off || !len || (payload_bytes && !payload)) return ZRC4_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        if (len[i] && (off[i] > payload_bytes || len[i] > payload_bytes - off[i]))
            return ZRC4_ERR_INVALID_ARG;
        // (ZRC4_IDLE_SLOT included: the kernels would skip it as padding)
        if (ids && ids[i] >= c->capacity) return ZRC4_ERR_SLOT_RANGE;
    }
    int rc = set_device(c);
    if (rc) return rc;
    // Several arbitrary ids: bucket them by 256-slot group here (the
    // zrc4_crypt_grouped contract), so every group's S-boxes move as one
    // coalesced image instead of 256 strided byte accesses per slot.  A slot
    // may appear once per call (as for every batched entry point).
    // Bucketing is one counting pass over the groups (r06; a comparison sort
    // of the ids cost 91 ms at 524 288 entries, more than the copies): bucket
    // b = the b-th group with entries, in ascending group order, its entries in
    // call order; a 256-bit mask per group finds a repeated slot.
    const bool grouped = ids && n > 1;
    std::vector<uint32_t> bgroup, bstart;     // bgroup: each bucket's group, declared to the kernel
    uint32_t buckets = 0;
    if (grouped) {
        const uint32_t ngroups = c->capacity / zrc4::kGroup;
        std::vector<uint64_t> seen((size_t)ngroups * 4, 0);
        bstart.assign(ngroups, ZRC4_IDLE_SLOT);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t g = ids[i] >> 8, k = ids[i] & 255u;
            uint64_t &w = seen[(size_t)g * 4 + (k >> 6)];
            if (w >> (k & 63u) & 1u) return ZRC4_ERR_INVALID_ARG;
            w |= 1ull << (k & 63u);
            bstart[g] = 0;
        }
        for (uint32_t g = 0; g < ngroups; ++g)
            if (bstart[g] != ZRC4_IDLE_SLOT) {
                bstart[g] = buckets++ * zrc4::kGroup;
                bgroup.push_back(g);
            }
    }
    const uint32_t m = grouped ? buckets * zrc4::kGroup : n;      // entries the kernel sees
    const size_t o_ids = 0, s_ids = ids ? align16((size_t)m * 4) : 0;
    const size_t o_off = o_ids + s_ids, s_off = align16((size_t)m * 8);
    const size_t o_len = o_off + s_off, s_len = align16((size_t)m * 4);
    const size_t o_pay = o_len + s_len, total = o_pay + align16(payload_bytes ? payload_bytes : 1);
    if ((rc = grow_stage(c, total))) return rc;
    if (grouped) {
        uint32_t *bi = reinterpret_cast<uint32_t *>(c->h_stage + o_ids);
        uint64_t *bo = reinterpret_cast<uint64_t *>(c->h_stage + o_off);
        uint32_t *bl = reinterpret_cast<uint32_t *>(c->h_stage + o_len);
        for (uint32_t e = 0; e < m; ++e) {
            bi[e] = ZRC4_IDLE_SLOT;
            bo[e] = 0;
            bl[e] = 0;
        }
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t e = bstart[ids[i] >> 8]++;     // (at most 256 per group: no slot twice)
            bi[e] = ids[i];
            bo[e] = off[i];
            bl[e] = len[i];
        }
    } else {
        if (ids) memcpy(c->h_stage + o_ids, ids, (size_t)n * 4);
        memcpy(c->h_stage + o_off, off, (size_t)n * 8);
        memcpy(c->h_stage + o_len, len, (size_t)n * 4);
    }
    // Small batches (the per-call RC4Encryption::encryption drop-in) run on
    // the pinned staging copy in place: no H2D / D2H copies on the latency
    // path.  Large ones are copied so the kernel streams HBM, not PCIe; from
    // 2 chunks of kPipeChunk on, the payload moves chunk by chunk so each
    // chunk's host copy overlaps the previous chunk's DMA (and, on the way
    // back, the next chunk's DMA overlaps this chunk's host copy).
    const bool zero_copy = total <= kZeroCopyMax;
    const bool piped = !zero_copy && payload_bytes >= 2 * kPipeChunk;
    uint8_t *st = c->h_stage;
    if (piped) {
        // (a failed enqueue returns only once the chunks already queued have
        // left the staging buffer, which the next call rewrites)
        bool ok = hipMemcpyAsync(c->d_stage, c->h_stage, o_pay, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        for (size_t a = 0; ok && a < payload_bytes; a += kPipeChunk) {
            const size_t l = std::min(kPipeChunk, payload_bytes - a);
            par_memcpy(c->h_stage + o_pay + a, payload + a, l);
            ok = hipMemcpyAsync(c->d_stage + o_pay + a, c->h_stage + o_pay + a, l, hipMemcpyHostToDevice,
                                c->stream) == hipSuccess;
        }
        if (!ok) {
            (void)hipStreamSynchronize(c->stream);
            return ZRC4_ERR_HIP;
        }
        st = c->d_stage;
    } else {
        if (payload_bytes) par_memcpy(c->h_stage + o_pay, payload, payload_bytes);
        if (!zero_copy) {
            ZRC4_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, total, hipMemcpyHostToDevice, c->stream));
            st = c->d_stage;
        }
    }
    CryptCall k = crypt_call(grouped ? zrc4::kGrouped : ids ? zrc4::kIds : zrc4::kRange,
                             ids ? (const uint32_t *)(st + o_ids) : nullptr, 0, st + o_pay,
                             (const uint64_t *)(st + o_off), (const uint32_t *)(st + o_len), m);
    k.decl = grouped ? bgroup.data() : nullptr;
    k.trusted = true;
    rc = launch_crypt(c, k, c->stream);
    if (rc) {
        // whatever was queued before the failure (the H2D copies, a check
        // kernel reading the zero-copy tables) still reads the staging
        // buffer, which the next call rewrites: drain it first
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    if (piped) return copy_back_piped(c, payload, o_pay, payload_bytes);
    if (payload_bytes && !zero_copy &&
        hipMemcpyAsync(c->h_stage + o_pay, c->d_stage + o_pay, payload_bytes, hipMemcpyDeviceToHost,
                       c->stream) != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return ZRC4_ERR_HIP;
    }
    rc = check_err(c, c->stream);
    if (rc) return rc;
    if (payload_bytes) par_memcpy(payload, c->h_stage + o_pay, payload_bytes);
    return ZRC4_OK;
}

int zrc4_make_sbox(zrc4_ctx *c, uint32_t id, const uint8_t *key, size_t keylen)
{
    if (!c || (keylen && !key)) return ZRC4_ERR_INVALID_ARG;
    if (id >= c->capacity) return ZRC4_ERR_SLOT_RANGE;
    // Only the first 256 key bytes can reach the S-box (the KSA runs i = 0..255
    // and reads key[i % len], rc4_encryption.h:60-70).
    const size_t kl = keylen > 256 ? 256 : keylen;
    const uint64_t ko = 0;
    const uint32_t kl32 = (uint32_t)kl;
    return zrc4_ksa_host(c, &id, key, kl, &ko, &kl32, 1);
}

int zrc4_encryption(zrc4_ctx *c, uint32_t id, uint8_t *data, int length)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (id >= c->capacity) return ZRC4_ERR_SLOT_RANGE;
    if (length <= 0) return ZRC4_OK;  // for (i = 0; i < length; ...) never runs (:81)
    if (!data) return ZRC4_ERR_INVALID_ARG;
    const uint64_t o = 0;
    const uint32_t l = (uint32_t)length;
    return zrc4_crypt_host(c, &id, data, (size_t)length, &o, &l, 1);
}

int zrc4_get_state(zrc4_ctx *c, uint32_t id, uint8_t sbox[256], uint8_t *x, uint8_t *y)
{
    if (!c || !sbox || !x || !y) return ZRC4_ERR_INVALID_ARG;
    if (id >= c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(c);
    if (rc) return rc;
    const uint8_t *img = c->arena + (size_t)(id >> 8) * zrc4::kGroupBytes;
    const uint32_t j = id & 255u, w = j >> 6, l = j & 63u;
    const uint32_t col = ((l & 31u) << 2) | (l >> 5) | ((w & 1u) << 1) | ((w >> 1) << 7);
    ZRC4_TRY(hipMemcpy2DAsync(sbox, 1, img + col, 256, 1, 256, hipMemcpyDeviceToHost, c->stream));
    uint16_t v = 0;
    ZRC4_TRY(hipMemcpyAsync(&v, c->xy + id, 2, hipMemcpyDeviceToHost, c->stream));
    ZRC4_TRY(hipStreamSynchronize(c->stream));
    *x = (uint8_t)(v & 255u);
    *y = (uint8_t)(v >> 8);
    return ZRC4_OK;
}

int zrc4_set_state(zrc4_ctx *c, uint32_t id, const uint8_t sbox[256], uint8_t x, uint8_t y)
{
    if (!c || !sbox) return ZRC4_ERR_INVALID_ARG;
    if (id >= c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(c);
    if (rc) return rc;
    uint8_t *img = c->arena + (size_t)(id >> 8) * zrc4::kGroupBytes;
    const uint32_t j = id & 255u, w = j >> 6, l = j & 63u;
    const uint32_t col = ((l & 31u) << 2) | (l >> 5) | ((w & 1u) << 1) | ((w >> 1) << 7);
    uint8_t tmp[258];
    memcpy(tmp, sbox, 256);
    const uint16_t v = (uint16_t)(x | (y << 8));
    ZRC4_TRY(hipMemcpy2DAsync(img + col, 256, tmp, 1, 1, 256, hipMemcpyHostToDevice, c->stream));
    ZRC4_TRY(hipMemcpyAsync(c->xy + id, &v, 2, hipMemcpyHostToDevice, c->stream));
    ZRC4_TRY(hipStreamSynchronize(c->stream));
    return ZRC4_OK;
}

int zrc4_get_states(zrc4_ctx *c, uint32_t first_slot, uint32_t n, uint8_t *sbox, uint8_t *x, uint8_t *y)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!sbox || !x || !y) return ZRC4_ERR_INVALID_ARG;
    if ((uint64_t)first_slot + n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(c);
    if (rc) return rc;
    const uint32_t g0 = first_slot / zrc4::kGroup, g1 = (first_slot + n - 1) / zrc4::kGroup;
    std::vector<uint8_t> img;
    std::vector<uint16_t> v(n);
    try {
        img.resize((size_t)(g1 - g0 + 1) * zrc4::kGroupBytes);
    } catch (const std::bad_alloc &) {
        return ZRC4_ERR_OUT_OF_MEMORY;
    }
    ZRC4_TRY(hipMemcpyAsync(img.data(), c->arena + (size_t)g0 * zrc4::kGroupBytes, img.size(), hipMemcpyDeviceToHost,
                            c->stream));
    ZRC4_TRY(hipMemcpyAsync(v.data(), c->xy + first_slot, (size_t)n * 2u, hipMemcpyDeviceToHost, c->stream));
    ZRC4_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = first_slot + i, j = id & 255u;
        const uint8_t *g = img.data() + (size_t)(id / zrc4::kGroup - g0) * zrc4::kGroupBytes + zrc4::col_of(j);
        uint8_t *o = sbox + (size_t)i * 256u;
        for (uint32_t k = 0; k < 256u; ++k) o[k] = g[k << 8];
        x[i] = (uint8_t)(v[i] & 255u);
        y[i] = (uint8_t)(v[i] >> 8);
    }
    return ZRC4_OK;
}

int zrc4_export_states(zrc4_ctx *c, const uint32_t *ids, uint32_t first_slot, uint32_t n, uint8_t *sbox,
                       uint16_t *xy, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_export(c, ids, first_slot, n, sbox, xy, (hipStream_t)stream);
}

int zrc4_import_states(zrc4_ctx *c, const uint32_t *ids, uint32_t first_slot, uint32_t n, const uint8_t *sbox,
                       const uint16_t *xy, void *stream)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    int rc = set_device(c);
    if (rc) return rc;
    return launch_import(c, ids, first_slot, n, sbox, xy, nullptr, 0u, (hipStream_t)stream);
}

int zrc4_copy_states(zrc4_ctx *dst, const uint32_t *dst_ids, uint32_t dst_first, zrc4_ctx *src,
                     const uint32_t *src_ids, uint32_t src_first, uint32_t n, void *stream)
{
    if (!dst || !src || dst->device != src->device) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!dst_ids && (uint64_t)dst_first + n > dst->capacity) return ZRC4_ERR_SLOT_RANGE;
    if (!src_ids && (uint64_t)src_first + n > src->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(dst);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // One scratch for the whole call, never chunks: every source is exported
    // before the first destination is written.
    const size_t need = (size_t)n * ZRC4_STATE_BYTES;
    if (need > dst->copy_scratch_bytes) {
        ZRC4_TRY(hipStreamSynchronize(s));      // an earlier copy on this stream may still use the old scratch
        size_t want = 1u << 20;
        while (want < need) want <<= 1;
        void *p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess) return ZRC4_ERR_OUT_OF_MEMORY;
        if (dst->copy_scratch) (void)hipFree(dst->copy_scratch);
        dst->copy_scratch = static_cast<uint8_t *>(p);
        dst->copy_scratch_bytes = want;
    }
    if (dst->copy_ev_live && dst->copy_last != s) ZRC4_TRY(hipStreamWaitEvent(s, dst->copy_ev, 0));
    uint8_t *sb = dst->copy_scratch;
    uint16_t *xy = reinterpret_cast<uint16_t *>(sb + (size_t)n * 256u);
    if ((rc = launch_export(src, src_ids, src_first, n, sb, xy, s))) return rc;
    rc = launch_import(dst, dst_ids, dst_first, n, sb, xy, src_ids, src->capacity, s);
    // mark where the scratch is free again; without an event, wait here
    if (!dst->copy_ev && hipEventCreateWithFlags(&dst->copy_ev, hipEventDisableTiming) != hipSuccess)
        dst->copy_ev = nullptr;
    dst->copy_ev_live = dst->copy_ev && hipEventRecord(dst->copy_ev, s) == hipSuccess;
    dst->copy_last = s;
    if (!dst->copy_ev_live) (void)hipStreamSynchronize(s);
    return rc;
}

int zrc4_set_states(zrc4_ctx *c, uint32_t first_slot, uint32_t n, const uint8_t *sbox, const uint8_t *x,
                    const uint8_t *y)
{
    if (!c) return ZRC4_ERR_INVALID_ARG;
    if (n == 0) return ZRC4_OK;
    if (!sbox || !x || !y) return ZRC4_ERR_INVALID_ARG;
    if ((uint64_t)first_slot + n > c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(c);
    if (rc) return rc;
    const size_t o_xy = (size_t)n * 256u, total = align16(o_xy + (size_t)n * 2u);
    if ((rc = grow_stage(c, total))) return rc;
    par_memcpy(c->h_stage, sbox, o_xy);
    uint16_t *v = reinterpret_cast<uint16_t *>(c->h_stage + o_xy);
    for (uint32_t i = 0; i < n; ++i) v[i] = (uint16_t)(x[i] | (y[i] << 8));
    uint8_t *st = c->h_stage;
    if (total > kZeroCopyMax) {
        ZRC4_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, total, hipMemcpyHostToDevice, c->stream));
        st = c->d_stage;
    }
    rc = launch_import(c, nullptr, first_slot, n, st, reinterpret_cast<const uint16_t *>(st + o_xy), nullptr, 0u,
                       c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);     // a queued H2D still reads the staging buffer
        return rc;
    }
    return check_err(c, c->stream);
}

const char *zrc4_strerror(int code)
{
    switch (code) {
    case ZRC4_OK: return "ok";
    case ZRC4_ERR_INVALID_ARG: return "invalid argument";
    case ZRC4_ERR_NO_DEVICE: return "no usable gfx950 (MI355X) HIP device";
    case ZRC4_ERR_OUT_OF_MEMORY: return "device or pinned memory allocation failed";
    case ZRC4_ERR_LAUNCH: return "kernel launch failed";
    case ZRC4_ERR_SLOT_RANGE: return "slot id out of range (>= capacity)";
    case ZRC4_ERR_HIP: return "HIP runtime error";
    case ZRC4_ERR_GROUP: return "zrc4_crypt_grouped: a 256-entry bucket mixes slot groups";
    case ZRC4_ERR_INTERNAL: return "internal error: S-box image not at LDS offset 0";
    case ZRC4_ERR_STATE: return "slot state lost (a failed reservoir crypt): reseed it with zrc4_ks_make_sbox or zrc4_ks_copy";
    default: return "unknown zrc4 error";
    }
}

// The product's string, plus " [NAME=value]" for each of the five build knobs
// (zsummerx_amd/build.py KEPT_KNOBS) that differs from its default, so that a
// test or diagnostic library cannot pass for the product.  (The defaults are
// repeated here from the knobs' #ifndef sites: tests/test_capi.py fails on
// the product library if one of them moves alone.)
#define ZRC4_STR2(x) #x
#define ZRC4_STR(x) ZRC4_STR2(x)
#define ZRC4_KNOB(NAME) " [" #NAME "=" ZRC4_STR(NAME) "]"
#if ZRC4_TIMING != 0
#define ZRC4_V_TIMING ZRC4_KNOB(ZRC4_TIMING)
#else
#define ZRC4_V_TIMING ""
#endif
#if ZRC4_WIN_TAG_LIMIT != (1u << 23)
#define ZRC4_V_WIN_TAG_LIMIT ZRC4_KNOB(ZRC4_WIN_TAG_LIMIT)
#else
#define ZRC4_V_WIN_TAG_LIMIT ""
#endif
#if defined(ZRC4_TEST_HOOKS) && ZRC4_TEST_HOOKS
#define ZRC4_V_TEST_HOOKS ZRC4_KNOB(ZRC4_TEST_HOOKS)
#else
#define ZRC4_V_TEST_HOOKS ""
#endif
#if ZRC4_GR_PRECLAIM_MAX != 64
#define ZRC4_V_GR_PRECLAIM_MAX ZRC4_KNOB(ZRC4_GR_PRECLAIM_MAX)
#else
#define ZRC4_V_GR_PRECLAIM_MAX ""
#endif
#if ZRC4_STATES_GATHER_MAX != 4
#define ZRC4_V_STATES_GATHER_MAX ZRC4_KNOB(ZRC4_STATES_GATHER_MAX)
#else
#define ZRC4_V_STATES_GATHER_MAX ""
#endif

const char *zrc4_version(void)
{
    return "zrc4-mi355x 0.2 (gfx950)" ZRC4_V_TIMING ZRC4_V_WIN_TAG_LIMIT ZRC4_V_TEST_HOOKS ZRC4_V_GR_PRECLAIM_MAX
           ZRC4_V_STATES_GATHER_MAX;
}

#if ZRC4_TIMING
// Diagnostic builds only: the per-wave timestamp records (zrc4_kernels.hpp,
// Stamps) live in the context's sink buffer.
int zrc4_debug_sink(zrc4_ctx *c, void **out)
{
    if (!c || !out) return ZRC4_ERR_INVALID_ARG;
    *out = c->sink;
    return ZRC4_OK;
}
#endif

}  // extern "C"

#include "zrc4_ks.inc"   // keystream reservoirs (zrc4_ks_*)
