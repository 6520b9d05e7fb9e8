// plan_check -- zsummerx_amd/csrc/zrc4_plan.hpp on the host alone (g++, no HIP).
//
//   plan_check           every row of the table below against plan_crypt
//   plan_check sweep     plan every shape of the sweep (tests/test_crypt_plan.py
//                        compares the names with the kernels of libzrc4.so):
//                        a plan without an error must name a form that exists;
//                        prints each kernel name reached, once
//   plan_check classes   the family of every in-place, undeclared range and
//                        grouped shape of the sweep, one per line:
//                        mode first_aligned G cus frame family
//                        (tests/test_crypt_plan.py: kernel_class of
//                        tests/dispatch_model.py says the same)
//   plan_check plan ...  the plan of each shape given on the command line
//                        (tests/test_gpu_addressing.py checks family() of
//                        tests/dispatch_model.py against it)
//
// The table's expectations are written out by hand from the rules the
// dispatch had as one if-chain in zrc4.hip; none is computed by plan_crypt.
#include "zrc4_plan.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>

using namespace zrc4;

namespace {

constexpr int kNoDecl = 0, kDeclared = 1, kTrusted = 2;
constexpr uint32_t kLast = 77;     // entries of the last group of a table row (ragged)

struct Row {
    const char *what;
    // the shape: n = (G - 1) * 256 + kLast, unless n is given
    int mode;
    bool first_aligned;
    uint32_t G, n, cus;
    bool frame;
    int decl;
    int io;
    uint32_t rounds;
    // the plan
    int err;
    int family;
    const char *name;
    uint32_t grid, block;
    int pre;
    uint32_t pre_grid;
    bool check, split;
};

constexpr int R = kRange, Gm = kGrouped, I = kIds;
constexpr int IP = kIoInPlace, KS = kIoKs, TO = kIoTo, TR = kIoToRounds;
constexpr int OK = kPlanOk, BAD = kPlanInvalidArg;
constexpr int WIN = kFamWin, DECL = kFamDecl, HALF = kFamHalf, WHOLE = kFamWhole, STREAM = kFamStream;
constexpr int NONE = kPreNone, FILL = kPreFill, COPY = kPreCopy;

const Row kTable[] = {
    // ---- 256 CUs, in place: aligned range
    {"range G=1", R, true, 1, 0, 256, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<1,0,0,0>", 64, 64, NONE, 0, false, false},
    {"range G=32", R, true, 32, 0, 256, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<1,0,0,0>", 2048, 64, NONE, 0, false, false},
    {"range G=33", R, true, 33, 0, 256, false, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<1,0,0>", 65, 256, NONE, 0, false, false},
    {"range G=128", R, true, 128, 0, 256, false, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<1,0,0>", 255, 256, NONE, 0, false, false},
    {"range G=129", R, true, 129, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<1,0,0>", 129, 256, NONE, 0, false, false},
    {"range G=256", R, true, 256, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<1,0,0>", 256, 256, NONE, 0, false, false},
    {"range G=257", R, true, 257, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,0,0>", 257, 256, NONE, 0, false, false},
    {"range G=600", R, true, 600, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,0,0>", 512, 256, NONE, 0, false, false},
    {"range n=32*256+1", R, true, 0, 32 * 256 + 1, 256, false, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<1,0,0>", 65, 256, NONE, 0, false, false},
    // ---- grouped
    {"grouped G=1", Gm, false, 1, 0, 256, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<2,0,0,0>", 64, 64, NONE, 0, false, false},
    {"grouped G=32", Gm, false, 32, 0, 256, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<2,0,0,0>", 2048, 64, NONE, 0, false, false},
    {"grouped G=33", Gm, false, 33, 0, 256, false, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<2,0,0>", 66, 256, NONE, 0, false, false},
    {"grouped G=128", Gm, false, 128, 0, 256, false, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<2,0,0>", 256, 256, NONE, 0, false, false},
    {"grouped G=129", Gm, false, 129, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<2,0,0>", 129, 256, NONE, 0, false, false},
    {"grouped G=256", Gm, false, 256, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<2,0,0>", 256, 256, NONE, 0, false, false},
    {"grouped G=257", Gm, false, 257, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, NONE, 0, false, false},
    {"grouped G=600", Gm, false, 600, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 512, 256, NONE, 0, false, false},
    // ---- a range from slot 37, scattered ids
    {"range fs37 G=5", R, false, 5, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<1,0,0>", 5, 256, NONE, 0, false, false},
    {"range fs37 G=257", R, false, 257, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<0,0,0>", 257, 256, NONE, 0, false, false},
    {"ids G=5", I, false, 5, 0, 256, false, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<0,0,0>", 5, 256, NONE, 0, false, false},
    {"ids G=257", I, false, 257, 0, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<0,0,0>", 257, 256, NONE, 0, false, false},
    // ---- write-only keystream
    {"ks range G=6", R, true, 6, 0, 256, false, kNoDecl, KS, 1, OK, WIN, "crypt_win_kernel<1,0,0,1>", 384, 64, NONE, 0, false, false},
    {"ks grouped G=6", Gm, false, 6, 0, 256, false, kNoDecl, KS, 1, OK, WIN, "crypt_win_kernel<2,0,0,1>", 384, 64, NONE, 0, false, false},
    {"ks grouped declared G=6", Gm, false, 6, 0, 256, false, kDeclared, KS, 1, OK, WIN, "crypt_win_kernel<2,0,1,1>", 384, 64, NONE, 0, false, false},
    {"ks range G=40", R, true, 40, 0, 256, false, kNoDecl, KS, 1, OK, HALF, "crypt_half_kernel<1,0,1>", 79, 256, NONE, 0, false, false},
    {"ks grouped G=40", Gm, false, 40, 0, 256, false, kNoDecl, KS, 1, OK, HALF, "crypt_half_kernel<2,0,1>", 80, 256, NONE, 0, false, false},
    {"ks range G=200", R, true, 200, 0, 256, false, kNoDecl, KS, 1, OK, WHOLE, "crypt_kernel<1,0,1>", 200, 256, NONE, 0, false, false},
    {"ks grouped G=200", Gm, false, 200, 0, 256, false, kNoDecl, KS, 1, OK, WHOLE, "crypt_kernel<2,0,1>", 200, 256, NONE, 0, false, false},
    {"ks grouped trusted G=200", Gm, false, 200, 0, 256, false, kTrusted, KS, 1, OK, DECL, "crypt_decl_kernel<0,0,1>", 200, 256, NONE, 0, false, false},
    {"ks range G=257", R, true, 257, 0, 256, false, kNoDecl, KS, 1, OK, STREAM, "crypt_stream_kernel<1,0,0>", 257, 256, FILL, 4096, false, false},
    {"ks range fs37 G=257", R, false, 257, 0, 256, false, kNoDecl, KS, 1, OK, STREAM, "crypt_stream_kernel<0,0,0>", 257, 256, FILL, 4096, false, false},
    {"ks grouped G=257", Gm, false, 257, 0, 256, false, kNoDecl, KS, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, FILL, 4096, false, false},
    {"ks grouped trusted G=257", Gm, false, 257, 0, 256, false, kTrusted, KS, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, FILL, 4096, false, false},
    // ---- out of place
    {"to range G=6", R, true, 6, 0, 256, false, kNoDecl, TO, 1, OK, WIN, "crypt_win_kernel<1,0,0,2>", 384, 64, NONE, 0, false, false},
    {"to grouped G=6", Gm, false, 6, 0, 256, false, kNoDecl, TO, 1, OK, WIN, "crypt_win_kernel<2,0,0,2>", 384, 64, NONE, 0, false, false},
    {"to grouped declared G=6", Gm, false, 6, 0, 256, false, kDeclared, TO, 1, OK, WIN, "crypt_win_kernel<2,0,1,2>", 384, 64, NONE, 0, false, false},
    {"to range G=40", R, true, 40, 0, 256, false, kNoDecl, TO, 1, OK, HALF, "crypt_half_kernel<1,0,2>", 79, 256, NONE, 0, false, false},
    {"to grouped G=40", Gm, false, 40, 0, 256, false, kNoDecl, TO, 1, OK, HALF, "crypt_half_kernel<2,0,2>", 80, 256, NONE, 0, false, false},
    {"to grouped declared G=40", Gm, false, 40, 0, 256, false, kDeclared, TO, 1, OK, DECL, "crypt_decl_kernel<0,1,2>", 80, 256, NONE, 0, false, false},
    {"to range G=200", R, true, 200, 0, 256, false, kNoDecl, TO, 1, OK, WHOLE, "crypt_kernel<1,0,2>", 200, 256, NONE, 0, false, false},
    {"to grouped G=200", Gm, false, 200, 0, 256, false, kNoDecl, TO, 1, OK, WHOLE, "crypt_kernel<2,0,2>", 200, 256, NONE, 0, false, false},
    {"to grouped declared G=200", Gm, false, 200, 0, 256, false, kDeclared, TO, 1, OK, DECL, "crypt_decl_kernel<0,0,2>", 200, 256, NONE, 0, false, false},
    {"to range G=257", R, true, 257, 0, 256, false, kNoDecl, TO, 1, OK, STREAM, "crypt_stream_kernel<1,0,0>", 257, 256, COPY, 4096, false, false},
    {"to grouped G=257", Gm, false, 257, 0, 256, false, kNoDecl, TO, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, COPY, 4096, false, false},
    {"to grouped declared G=257", Gm, false, 257, 0, 256, false, kDeclared, TO, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, COPY, 4096, true, false},
    // ---- rounds: never the window kernel; past the CU count, one kIoTo call per round
    {"rounds range G=6", R, true, 6, 0, 256, false, kNoDecl, TR, 2, OK, HALF, "crypt_half_kernel<1,0,3>", 11, 256, NONE, 0, false, false},
    {"rounds grouped G=6", Gm, false, 6, 0, 256, false, kNoDecl, TR, 2, OK, HALF, "crypt_half_kernel<2,0,3>", 12, 256, NONE, 0, false, false},
    {"rounds declared G=6", Gm, false, 6, 0, 256, false, kDeclared, TR, 2, OK, DECL, "crypt_decl_kernel<0,1,3>", 12, 256, NONE, 0, false, false},
    {"rounds range fs37 G=6", R, false, 6, 0, 256, false, kNoDecl, TR, 2, OK, WHOLE, "crypt_kernel<1,0,3>", 6, 256, NONE, 0, false, false},
    {"rounds range G=200", R, true, 200, 0, 256, false, kNoDecl, TR, 64, OK, WHOLE, "crypt_kernel<1,0,3>", 200, 256, NONE, 0, false, false},
    {"rounds grouped G=200", Gm, false, 200, 0, 256, false, kNoDecl, TR, 64, OK, WHOLE, "crypt_kernel<2,0,3>", 200, 256, NONE, 0, false, false},
    {"rounds declared G=200", Gm, false, 200, 0, 256, false, kDeclared, TR, 64, OK, DECL, "crypt_decl_kernel<0,0,3>", 200, 256, NONE, 0, false, false},
    {"rounds range G=257", R, true, 257, 0, 256, false, kNoDecl, TR, 3, OK, STREAM, "crypt_stream_kernel<1,0,0>", 257, 256, COPY, 4096, false, true},
    {"rounds grouped G=257", Gm, false, 257, 0, 256, false, kNoDecl, TR, 3, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, COPY, 4096, false, true},
    {"rounds declared G=257", Gm, false, 257, 0, 256, false, kDeclared, TR, 3, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, COPY, 4096, true, true},
    {"rounds trusted G=257", Gm, false, 257, 0, 256, false, kTrusted, TR, 3, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, COPY, 4096, false, true},
    {"rounds n*rounds = 0xFFF00000", R, true, 0, 0xFFF0000u, 256, false, kNoDecl, TR, 16, OK, STREAM, "crypt_stream_kernel<1,0,0>", 512, 256, COPY, 4096, false, true},
    // ---- a frame with every family
    {"frame range G=3", R, true, 3, 0, 256, true, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<1,1,0,0>", 192, 64, NONE, 0, false, false},
    {"frame grouped G=6", Gm, false, 6, 0, 256, true, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<2,1,0,0>", 384, 64, NONE, 0, false, false},
    {"frame declared G=6", Gm, false, 6, 0, 256, true, kDeclared, IP, 1, OK, WIN, "crypt_win_kernel<2,1,1,0>", 384, 64, NONE, 0, false, false},
    {"frame declared G=40", Gm, false, 40, 0, 256, true, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<1,1,0>", 80, 256, NONE, 0, false, false},
    {"frame declared G=200", Gm, false, 200, 0, 256, true, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<1,0,0>", 200, 256, NONE, 0, false, false},
    {"frame range G=33", R, true, 33, 0, 256, true, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<1,1,0>", 65, 256, NONE, 0, false, false},
    {"frame grouped G=40", Gm, false, 40, 0, 256, true, kNoDecl, IP, 1, OK, HALF, "crypt_half_kernel<2,1,0>", 80, 256, NONE, 0, false, false},
    {"frame range G=129", R, true, 129, 0, 256, true, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<1,1,0>", 129, 256, NONE, 0, false, false},
    {"frame range fs37 G=5", R, false, 5, 0, 256, true, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<1,1,0>", 5, 256, NONE, 0, false, false},
    {"frame grouped G=200", Gm, false, 200, 0, 256, true, kNoDecl, IP, 1, OK, WHOLE, "crypt_kernel<2,1,0>", 200, 256, NONE, 0, false, false},
    {"frame range G=257", R, true, 257, 0, 256, true, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,0,1>", 257, 256, NONE, 0, false, false},
    {"frame grouped G=257", Gm, false, 257, 0, 256, true, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,1>", 257, 256, NONE, 0, false, false},
    {"frame range fs37 G=260", R, false, 260, 0, 256, true, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<0,0,1>", 260, 256, NONE, 0, false, false},
    // ---- declared groups, untrusted and trusted
    {"declared G=6", Gm, false, 6, 0, 256, false, kDeclared, IP, 1, OK, WIN, "crypt_win_kernel<2,0,1,0>", 384, 64, NONE, 0, false, false},
    {"trusted G=6", Gm, false, 6, 0, 256, false, kTrusted, IP, 1, OK, WIN, "crypt_win_kernel<2,0,1,0>", 384, 64, NONE, 0, false, false},
    {"declared G=40", Gm, false, 40, 0, 256, false, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<0,1,0>", 80, 256, NONE, 0, false, false},
    {"trusted G=40", Gm, false, 40, 0, 256, false, kTrusted, IP, 1, OK, DECL, "crypt_decl_kernel<0,1,0>", 80, 256, NONE, 0, false, false},
    {"declared G=128", Gm, false, 128, 0, 256, false, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<0,1,0>", 256, 256, NONE, 0, false, false},
    {"declared G=129", Gm, false, 129, 0, 256, false, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<0,0,0>", 129, 256, NONE, 0, false, false},
    {"declared G=200", Gm, false, 200, 0, 256, false, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<0,0,0>", 200, 256, NONE, 0, false, false},
    {"trusted G=200", Gm, false, 200, 0, 256, false, kTrusted, IP, 1, OK, DECL, "crypt_decl_kernel<0,0,0>", 200, 256, NONE, 0, false, false},
    {"declared G=256", Gm, false, 256, 0, 256, false, kDeclared, IP, 1, OK, DECL, "crypt_decl_kernel<0,0,0>", 256, 256, NONE, 0, false, false},
    {"trusted G=256", Gm, false, 256, 0, 256, false, kTrusted, IP, 1, OK, DECL, "crypt_decl_kernel<0,0,0>", 256, 256, NONE, 0, false, false},
    {"declared G=257", Gm, false, 257, 0, 256, false, kDeclared, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, NONE, 0, true, false},
    {"trusted G=257", Gm, false, 257, 0, 256, false, kTrusted, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 257, 256, NONE, 0, false, false},
    {"declared on a range call: ignored", R, true, 40, 0, 256, false, kDeclared, IP, 1, OK, HALF, "crypt_half_kernel<1,0,0>", 79, 256, NONE, 0, false, false},
    // ---- 8 CUs: the window kernel ahead of the stream test; check + stream
    {"8 CUs range G=20", R, true, 20, 0, 8, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<1,0,0,0>", 1280, 64, NONE, 0, false, false},
    {"8 CUs grouped G=20", Gm, false, 20, 0, 8, false, kNoDecl, IP, 1, OK, WIN, "crypt_win_kernel<2,0,0,0>", 1280, 64, NONE, 0, false, false},
    {"8 CUs declared G=33", Gm, false, 33, 0, 8, false, kDeclared, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 16, 256, NONE, 0, true, false},
    {"8 CUs ks range fs37 G=9", R, false, 9, 0, 8, false, kNoDecl, KS, 1, OK, STREAM, "crypt_stream_kernel<0,0,0>", 9, 256, FILL, 128, false, false},
    // ---- 600 CUs: the up-front check ahead of the half-group kernel
    {"600 CUs declared G=280", Gm, false, 280, 0, 600, false, kDeclared, IP, 1, OK, HALF, "crypt_half_kernel<2,0,0>", 560, 256, NONE, 0, true, false},
    {"600 CUs trusted G=280", Gm, false, 280, 0, 600, false, kTrusted, IP, 1, OK, HALF, "crypt_half_kernel<2,0,0>", 560, 256, NONE, 0, false, false},
    {"600 CUs declared G=400", Gm, false, 400, 0, 600, false, kDeclared, IP, 1, OK, WHOLE, "crypt_kernel<2,0,0>", 400, 256, NONE, 0, true, false},
    // ---- the 32-bit entry-index limit of the grouped stream kernel
    {"grouped n = 0xFFF00000", Gm, false, 0, 0xFFF00000u, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,1,0>", 512, 256, NONE, 0, false, false},
    {"grouped n = 0xFFF00001", Gm, false, 0, 0xFFF00001u, 256, false, kNoDecl, IP, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"range n = 0xFFF00001", R, true, 0, 0xFFF00001u, 256, false, kNoDecl, IP, 1, OK, STREAM, "crypt_stream_kernel<1,0,0>", 512, 256, NONE, 0, false, false},
    // ---- refused arguments
    {"ks + frame", R, true, 6, 0, 256, true, kNoDecl, KS, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"to + frame", Gm, false, 40, 0, 256, true, kNoDecl, TO, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"rounds + frame", R, true, 200, 0, 256, true, kNoDecl, TR, 2, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"ks + ids", I, false, 5, 0, 256, false, kNoDecl, KS, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"to + ids", I, false, 257, 0, 256, false, kNoDecl, TO, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"rounds + ids", I, false, 5, 0, 256, false, kNoDecl, TR, 2, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"rounds = 1", R, true, 6, 0, 256, false, kNoDecl, TR, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"rounds = 0", Gm, false, 6, 0, 256, false, kNoDecl, TR, 0, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"rounds n*rounds = 0xFFF00010", R, true, 0, 0xFFF0001u, 256, false, kNoDecl, TR, 16, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"ids + frame G=5", I, false, 5, 0, 256, true, kNoDecl, IP, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
    {"ids + frame G=257", I, false, 257, 0, 256, true, kNoDecl, IP, 1, BAD, 0, "", 0, 0, NONE, 0, false, false},
};

CryptShape shape(int mode, bool first_aligned, uint32_t n, uint32_t cus, bool frame, int decl, int io, uint32_t rounds)
{
    CryptShape s{};
    s.mode = mode;
    s.first_aligned = first_aligned;
    s.n = n;
    s.rounds = rounds;
    s.cus = cus;
    s.frame = frame;
    s.declared = decl != kNoDecl;
    s.trusted = decl == kTrusted;
    s.io = io;
    return s;
}

int check_table()
{
    int bad = 0, rows = 0;
    for (const Row &r : kTable) {
        ++rows;
        const uint32_t n = r.n ? r.n : (r.G - 1u) * 256u + kLast;
        const CryptPlan p = plan_crypt(shape(r.mode, r.first_aligned, n, r.cus, r.frame, r.decl, r.io, r.rounds));
        bool ok = p.err == r.err;
        if (ok && p.err == kPlanOk)
            ok = p.family == r.family && !strcmp(p.name().s, r.name) && p.form_exists() && p.grid == r.grid &&
                 p.block == r.block && p.pre == r.pre && p.pre_grid == r.pre_grid && p.check == r.check &&
                 p.split == r.split && p.groups == (n + 255u) / 256u;
        if (!ok) {
            ++bad;
            printf("MISMATCH %s: err %d family %d %s grid %u block %u pre %d/%u check %d split %d\n", r.what, p.err,
                   p.family, p.err ? "" : p.name().s, p.grid, p.block, p.pre, p.pre_grid, (int)p.check, (int)p.split);
        }
    }
    printf("%d rows, %d mismatches\n", rows, bad);
    return bad ? 1 : 0;
}

// The sweep: every mode, aligned and not, G = 1..700 (a full and a one-entry
// last group), three CU counts, frame, the three declared states, every io,
// three round counts.
template <typename F>
void sweep(F &&f)
{
    static const uint32_t kCus[] = {8, 256, 304}, kRounds[] = {1, 2, 64};
    for (int mode : {I, R, Gm})
        for (int al = 0; al < 2; ++al)
            for (uint32_t G = 1; G <= 700; ++G)
                for (uint32_t n : {G * 256u - 255u, G * 256u})
                    for (uint32_t cus : kCus)
                        for (int frame = 0; frame < 2; ++frame)
                            for (int decl : {kNoDecl, kDeclared, kTrusted})
                                for (int io : {IP, KS, TO, TR})
                                    for (uint32_t rounds : kRounds)
                                        f(shape(mode, al != 0, n, cus, frame != 0, decl, io, rounds), G);
}

int check_sweep()
{
    std::set<std::string> names;
    long plans = 0, errors = 0, bad = 0;
    sweep([&](const CryptShape &s, uint32_t G) {
        const CryptPlan p = plan_crypt(s);
        ++plans;
        if (p.err != kPlanOk) {
            ++errors;
            return;
        }
        const bool sane = p.form_exists() && p.groups == G && p.grid > 0 && p.grid <= 64u * G &&
                          (p.block == 64 || p.block == 256) && (p.pre == kPreNone) == (p.pre_grid == 0);
        if (!sane) {
            if (bad++ < 10)
                fprintf(stderr, "no such form or grid: mode %d aligned %d n %u cus %u frame %d io %d -> %s grid %u\n",
                        s.mode, (int)s.first_aligned, s.n, s.cus, (int)s.frame, s.io, p.name().s, p.grid);
            return;
        }
        names.insert(p.name().s);
    });
    for (const std::string &k : names) printf("%s\n", k.c_str());
    fprintf(stderr, "%ld shapes, %ld refused, %ld without a form, %zu kernels\n", plans, errors, bad, names.size());
    return bad ? 1 : 0;
}

int print_classes()
{
    static const char *const kFam[] = {"win", "decl", "half", "whole", "stream"};
    sweep([&](const CryptShape &s, uint32_t G) {
        if (s.mode == I || s.io != IP || s.declared || s.rounds != 1 || s.n != G * 256u) return;
        const CryptPlan p = plan_crypt(s);
        printf("%d %d %u %u %d %s\n", s.mode, (int)s.first_aligned, G, s.cus, (int)s.frame,
               p.err ? "error" : kFam[p.family]);
    });
    return 0;
}

// plan_check plan <mode> <first_aligned> <n> <cus> <frame> <decl> <io> <rounds> ...
// (any number of such groups of eight): one line per shape,
//   family kernel-name pre split
// or "error" where plan_crypt refuses the shape.
int print_plans(int argc, char **argv)
{
    static const char *const kFam[] = {"win", "decl", "half", "whole", "stream"};
    if (argc < 8 || argc % 8) return 2;
    for (int a = 0; a < argc; a += 8) {
        unsigned long v[8];
        for (int i = 0; i < 8; ++i) v[i] = strtoul(argv[a + i], nullptr, 10);
        const CryptPlan p = plan_crypt(shape((int)v[0], v[1] != 0, (uint32_t)v[2], (uint32_t)v[3], v[4] != 0,
                                             (int)v[5], (int)v[6], (uint32_t)v[7]));
        if (p.err != kPlanOk)
            printf("error\n");
        else
            printf("%s %s %d %d\n", kFam[p.family], p.name().s, p.pre, (int)p.split);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) return check_table();
    if (!strcmp(argv[1], "sweep")) return check_sweep();
    if (!strcmp(argv[1], "classes")) return print_classes();
    if (!strcmp(argv[1], "plan")) return print_plans(argc - 2, argv + 2);
    fprintf(stderr, "usage: plan_check [sweep | classes | plan <8 numbers per shape>]\n");
    return 2;
}
