// zrc4_plan.hpp -- which crypt kernel a call launches, as a pure function.
//
// Plain C++17 over <stdint.h>: no HIP, no pointers, no context, so the choice
// compiles and is tested on the host alone (tests/cpp/plan_check.cpp).
// launch_crypt (zrc4.hip) fills a CryptShape, calls plan_crypt and carries the
// plan out; the *_form_exists predicates below are the one place where the
// set of crypt-family kernel instantiations is written down.
#pragma once
#include <stdint.h>

namespace zrc4 {

constexpr int kGroup = 256;            // slots per workgroup / arena group

// Addressing of a crypt batch (the slot of entry e); the kernels' side of each
// mode is described above crypt_body (zrc4_kernels.hpp).
enum CryptMode : int { kIds = 0, kRange = 1, kGrouped = 2 };

// The I/O form of a crypt kernel (last template parameter of the window, half-
// group, whole-group and declared kernels):
//   kIoInPlace  the span is read, XORed and written back (zrc4_crypt_*);
//   kIoKs       write-only keystream (zrc4_keystream_*): the span is stored
//               and never read;
//   kIoTo       out of place (zrc4_crypt_to_*): entry i reads its SOURCE span
//               and stores the XOR to its destination span; the destination
//               is never read and the source never written;
//   kIoToRounds kIoTo, `rounds` times in one launch (zrc4_crypt_to_*_rounds;
//               the lane-per-stream kernels only): the group image is loaded
//               and stored once, and each lane walks its slot's `rounds`
//               entries in order (crypt_body).
enum CryptIo : int { kIoInPlace = 0, kIoKs = 1, kIoTo = 2, kIoToRounds = 3 };

// Most buckets whose declared groups travel in the window kernel's arguments
// (WinGroups, zrc4_win.hpp), and the window kernel's largest launch.
constexpr uint32_t kWinMaxBuckets = 32;      // bench.py's WIN_MAX_GROUPS mirrors this constant
// The same for the half-group and whole-group kernels (BucketGroups,
// zrc4_kernels.hpp: 1 KiB of kernel arguments).
constexpr uint32_t kBodyMaxBuckets = 256;
// Half-group workgroups (kRange / kGrouped, few groups): one per CU;
// workgroup 2w + h runs half h of bucket w.  Launched with 256 threads, of
// which the two waves that work are picked by SIMD (crypt_body).
constexpr uint32_t kHalfBlock = 256u;

// Everything the choice depends on, and nothing it does not.
struct CryptShape {
    int mode;            // CryptMode
    bool first_aligned;  // kRange: first_slot % 256 == 0 (other modes: ignored)
    uint32_t n;          // entries (per round), > 0
    uint32_t rounds;     // kIoToRounds: entries per slot; otherwise ignored
    uint32_t cus;        // compute units of the device
    bool frame;          // the framing walk runs in the same launch
    bool declared;       // the caller declared every bucket's group (kGrouped)
    bool trusted;        // ... and they were computed here, from host ids
    int io;              // CryptIo
};

enum CryptFamily : int { kFamWin, kFamDecl, kFamHalf, kFamWhole, kFamStream };
enum CryptPre : int { kPreNone, kPreFill, kPreCopy };   // span_fill_kernel / span_copy_kernel in front
enum : int { kPlanOk = 0, kPlanInvalidArg = 1 };

// Which instantiations exist.  FRAME only in place; range and grouped in every
// I/O form, ids in the plain whole-group form alone.
constexpr bool io_exists(int io) { return io >= kIoInPlace && io <= kIoToRounds; }
constexpr bool lane_form_exists(int mode, bool frame, int io)      // one lane per stream
{
    return (mode == kRange || mode == kGrouped) && io_exists(io) && (!frame || io == kIoInPlace);
}
constexpr bool win_form_exists(int mode, bool frame, bool decl, int io)     // no rounds form
{
    return lane_form_exists(mode, frame, io) && io != kIoToRounds && (!decl || mode == kGrouped);
}
constexpr bool decl_form_exists(bool frame, bool /*half*/, int io) { return lane_form_exists(kGrouped, frame, io); }
constexpr bool half_form_exists(int mode, bool frame, int io) { return lane_form_exists(mode, frame, io); }
constexpr bool whole_form_exists(int mode, bool frame, int io)
{
    return lane_form_exists(mode, frame, io) || (mode == kIds && !frame && io == kIoInPlace);
}
constexpr bool stream_form_exists(bool pf, bool gr, bool /*frame*/) { return pf || !gr; }   // in place only

struct CryptPlan {
    int err = kPlanOk;                 // kPlanInvalidArg: nothing else is set
    int family = kFamWhole;
    // the family's template coordinates: win <mode,frame,decl,io>, decl
    // <frame,half,io>, half / whole <mode,frame,io>, stream <pf,gr,frame>
    int mode = kIds, io = kIoInPlace;
    bool frame = false, decl = false, half = false, pf = false, gr = false;
    uint32_t groups = 0;               // G: groups (range) or buckets (grouped) of 256 entries
    uint32_t grid = 0, block = 0;
    int pre = kPreNone;                // on the same stream, ahead of the kernel
    uint32_t pre_grid = 0;             // (its block: 256)
    bool check = false;                // decl_check_kernel (grid G, block 256) ahead of both
    bool split = false;                // kIoToRounds: `rounds` calls of kIoTo, each one this plan

    bool form_exists() const
    {
        switch (family) {
        case kFamWin: return win_form_exists(mode, frame, decl, io);
        case kFamDecl: return decl_form_exists(frame, half, io);
        case kFamHalf: return half_form_exists(mode, frame, io);
        case kFamWhole: return whole_form_exists(mode, frame, io);
        case kFamStream: return stream_form_exists(pf, gr, frame);
        }
        return false;
    }

    // The kernel's key as tools/isa_compare.py prints it (without the return
    // type and namespace), e.g. crypt_win_kernel<2,1,1,0>.
    struct Name {
        char s[40];
    };
    Name name() const
    {
        static constexpr const char *kBase[] = {"crypt_win_kernel", "crypt_decl_kernel", "crypt_half_kernel",
                                                "crypt_kernel", "crypt_stream_kernel"};
        int v[4], nv = 3;
        switch (family) {
        case kFamWin: v[0] = mode, v[1] = frame, v[2] = decl, v[3] = io, nv = 4; break;
        case kFamDecl: v[0] = frame, v[1] = half, v[2] = io; break;
        case kFamStream: v[0] = pf, v[1] = gr, v[2] = frame; break;
        default: v[0] = mode, v[1] = frame, v[2] = io; break;
        }
        Name out{};
        char *p = out.s;
        for (const char *b = kBase[family]; *b; ++b) *p++ = *b;
        for (int i = 0; i < nv; ++i) {
            *p++ = i ? ',' : '<';
            *p++ = (char)('0' + v[i]);      // every coordinate is one digit
        }
        *p++ = '>';
        return out;
    }
};

inline CryptPlan plan_invalid()
{
    CryptPlan p;
    p.err = kPlanInvalidArg;
    return p;
}

// The choice.  G = groups (range) or buckets (grouped) of 256 entries;
// "aligned" = every workgroup's 256 entries are one arena group's slots.
inline CryptPlan plan_crypt(const CryptShape &s)
{
    const bool grouped = s.mode == kGrouped, range = s.mode == kRange;
    const bool ks = s.io == kIoKs, to = s.io == kIoTo, tor = s.io == kIoToRounds;
    const bool aligned = grouped || (range && s.first_aligned);
    const bool decl = s.declared && grouped;
    const uint64_t G = ((uint64_t)s.n + kGroup - 1) / kGroup;
    // More groups than CUs: the persistent throughput kernel (2 workgroups
    // per CU, whole-line stores through the DPP transpose); otherwise one
    // group per workgroup (chain-bound, per-lane stores).  A/B: the DPP path
    // is 5-7 us slower at one group per CU (cfg2 56.1 vs 48.8 us, cfg3 28.1
    // vs 22.7 us; profiles/r02_ab_dpp_direct.log).
    const bool stream = G > s.cus;

    // 1. Arguments.  The write-only and out-of-place forms are never framed
    // and have no ids form; no ids kernel is framed.  The grouped stream
    // kernel computes entry indexes of the bucket after next in 32 bits, and
    // a rounds kernel indexes rounds * n table entries.
    if ((ks || to || tor) && (s.frame || s.mode == kIds)) return plan_invalid();
    if (tor && (s.rounds < 2u || (uint64_t)s.n * s.rounds > 0xFFF00000u)) return plan_invalid();
    if (grouped && stream && s.n > 0xFFF00000u) return plan_invalid();
    if (s.mode == kIds && s.frame) return plan_invalid();

    // 2. The persistent kernel has no out-of-place form, so no rounds form
    // either: one kIoTo call per round, each with claims of its own.
    if (tor && stream) {
        CryptShape one = s;
        one.io = kIoTo;
        one.rounds = 1;
        CryptPlan p = plan_crypt(one);
        p.split = true;
        return p;
    }

    CryptPlan p;
    p.mode = s.mode;
    p.frame = s.frame;
    p.io = s.io;
    p.groups = (uint32_t)G;
    p.block = kGroup;

    // 3. Few aligned groups (at most kWinMaxBuckets, so that declared groups
    // travel in WinGroups): 16 lanes per stream (speculative windows,
    // crypt_win_kernel), one wave per 4 streams, 64 workgroups per group:
    // ~46 cycles per byte against ~96 with one lane per stream (DESIGN.md
    // 3.8).  Ahead of the `stream` test on purpose: a device with fewer CUs
    // than G still takes it.  No rounds form: a rounds call of 32 groups and
    // fewer runs the lane-per-stream kernels
    // (profiles/crypt_to_rounds/crypt_to_rounds_bench_window_crossover.jsonl).
    if (!tor && G <= kWinMaxBuckets && aligned) {
        p.family = kFamWin;
        p.decl = decl;
        p.grid = 64u * (uint32_t)G;
        p.block = 64;
        return p;
    }
    // 4. Declared groups on the half-group / whole-group kernels (at most
    // kBodyMaxBuckets buckets, one bucket per CU): in the kernel arguments,
    // checked there, so the image leaves at kernel entry.
    if (decl && !stream && G <= kBodyMaxBuckets) {
        p.family = kFamDecl;
        p.half = 2u * G <= s.cus;
        p.grid = (uint32_t)(p.half ? 2u * G : G);
        return p;
    }
    // 5. Larger declared launches: decl_check_kernel first (stream-ordered),
    // which blocks the groups of a disagreeing bucket through the claims.
    // Trusted groups (computed here from host ids) skip it.
    p.check = decl && !s.trusted;
    // 6. Few whole groups: half-group workgroups, one per CU.  At 2 waves per
    // CU a chain step takes 41.2 us per KiB against 43.1 at 4
    // (profiles/r02/tl_waves.log).  A grouped bucket's slots may sit in
    // either half whatever its entry count, so it always gets both halves.
    if (2u * G <= s.cus && aligned) {
        p.family = kFamHalf;
        p.grid = grouped ? 2u * (uint32_t)G : (uint32_t)(((uint64_t)s.n + kGroup / 2 - 1) / (kGroup / 2));
        p.block = kHalfBlock;
        return p;
    }
    // 7. One group per workgroup, at most one per CU (an unaligned range and
    // scattered ids: each lane gathers and scatters its own column).
    if (!stream) {
        p.family = kFamWhole;
        p.grid = (uint32_t)G;
        return p;
    }
    // 8. The persistent kernel, in place.  PF: the prefetching form (aligned
    // batches), GR: its grouped form.  It has no write-only and no out-of-
    // place form: the spans are zeroed first (0 ^ k = k), or the sources
    // copied into the destinations, by a pre-kernel on the same stream (one
    // wave per entry, a few waves per SIMD at most).  With a frame, the
    // framing walk runs in each workgroup's tail over the chunks it decrypted.
    p.family = kFamStream;
    p.io = kIoInPlace;
    p.pf = aligned;
    p.gr = grouped;
    p.grid = (uint32_t)(G < 2u * (uint64_t)s.cus ? G : 2u * (uint64_t)s.cus);
    p.pre = ks ? kPreFill : to ? kPreCopy : kPreNone;
    if (p.pre != kPreNone) {
        const uint64_t want = ((uint64_t)s.n + 3u) / 4u, cap = 16u * (uint64_t)s.cus;
        p.pre_grid = (uint32_t)(want < cap ? want : cap);
    }
    return p;
}

}  // namespace zrc4
