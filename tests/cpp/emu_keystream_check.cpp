// emu_keystream_check.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_keystream_hooks.py).
// The CPU emulation of the write-only keystream calls (emu_zrc4_keystream.cpp
// over emu_zrc4_hip.cpp) against the oracle RC4 and the rules of
// include/zrc4.h: spans receive the slot's next keystream bytes whatever they
// held, bytes between spans and the spans of skipped entries (len 0, idle id)
// keep theirs, a following crypt continues each stream, and a bucket that
// names two groups is refused (ZRC4_ERR_GROUP, its slots not advanced) while
// the other buckets run.  Prints one line per case; exits non-zero on any
// mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zrc4.h"
extern "C" {
#include "rc4_oracle.h"
}

namespace {

constexpr uint8_t kFill = 0xA5;
const uint32_t kLens[] = {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 250};

struct Case {
    zrc4_ctx *c = nullptr;
    std::vector<oracle_rc4_state> ref;
    explicit Case(uint32_t slots) : ref(slots)
    {
        zrc4_create(&c, 0, slots);
        std::vector<uint32_t> ids(slots), kl(slots, 5);
        std::vector<uint64_t> ko(slots);
        std::vector<uint8_t> keys(slots * 5);
        for (uint32_t s = 0; s < slots; ++s) {
            ids[s] = s;
            ko[s] = 5ull * s;
            for (int k = 0; k < 5; ++k) keys[5 * s + k] = (uint8_t)(s * 7 + k * 31 + 1);
            oracle_make_sbox(&ref[s], &keys[5 * s], 5);
        }
        zrc4_ksa(c, ids.data(), keys.data(), ko.data(), kl.data(), slots, nullptr);
    }
    ~Case() { zrc4_destroy(c); }
};

// Expected buffer: kFill everywhere, oracle keystream in the spans of `run` entries.
bool spans_ok(const char *what, Case &k, const std::vector<uint32_t> &slot, const std::vector<uint8_t> &run,
              const std::vector<uint64_t> &off, const std::vector<uint32_t> &len, const std::vector<uint8_t> &out)
{
    std::vector<uint8_t> want(out.size(), kFill);
    for (size_t i = 0; i < slot.size(); ++i) {
        if (!run[i] || !len[i]) continue;
        std::memset(&want[off[i]], 0, len[i]);
        oracle_encryption(&k.ref[slot[i]], &want[off[i]], (long)len[i]);
    }
    const bool ok = want == out;
    std::printf("%s: %s\n", what, ok ? "ok" : "MISMATCH");
    return ok;
}

// A crypt of 8 bytes per slot after the keystream call: every stream goes on
// where the oracle's does (slots of a refused bucket: where they were).
bool continues_ok(const char *what, Case &k)
{
    const uint32_t n = (uint32_t)k.ref.size();
    std::vector<uint32_t> ids(n), len(n, 8);
    std::vector<uint64_t> off(n);
    std::vector<uint8_t> got(8u * n), want(8u * n);
    for (uint32_t s = 0; s < n; ++s) {
        ids[s] = s;
        off[s] = 8ull * s;
        for (int b = 0; b < 8; ++b) got[8 * s + b] = want[8 * s + b] = (uint8_t)(s + b);
        oracle_encryption(&k.ref[s], &want[8 * s], 8);
    }
    zrc4_crypt(k.c, ids.data(), got.data(), off.data(), len.data(), n, nullptr);
    const bool ok = got == want;
    std::printf("%s, following crypt: %s\n", what, ok ? "ok" : "MISMATCH");
    return ok;
}

int range_case()
{
    const uint32_t first = 3, n = 300;
    Case k(600);
    std::vector<uint32_t> slot(n), len(n);
    std::vector<uint64_t> off(n);
    std::vector<uint8_t> run(n, 1);
    uint64_t at = 5;
    for (uint32_t i = 0; i < n; ++i) {
        slot[i] = first + i;
        len[i] = kLens[i % 15];
        off[i] = at;
        at += len[i] + 1 + i % 3;                      // 1-3 guard bytes
    }
    std::vector<uint8_t> out(at + 8, kFill);
    const int rc = zrc4_keystream_range(k.c, first, out.data(), off.data(), len.data(), n, nullptr);
    bool ok = rc == ZRC4_OK;
    ok = spans_ok("range", k, slot, run, off, len, out) && ok;
    ok = continues_ok("range", k) && ok;
    return ok ? 0 : 1;
}

int grouped_case(bool declared, bool mixed)
{
    const uint32_t nb = 3;
    Case k(4 * 256);
    const uint32_t n = nb * 256;
    std::vector<uint32_t> ids(n, ZRC4_IDLE_SLOT), len(n), bg = {2, 0, ZRC4_IDLE_SLOT};
    std::vector<uint64_t> off(n);
    std::vector<uint8_t> run(n, 0);
    uint64_t at = 3;
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t e = 0; e < 256; ++e) {
            const uint32_t i = b * 256 + e;
            len[i] = kLens[(i + 1) % 15];
            off[i] = at;
            at += len[i] + 1 + i % 3;
            if (b < 2 && e % 3 != 2) {                 // bucket 2 and every third entry: idle ids
                ids[i] = bg[b] * 256 + (e * 37 + 11) % 256;      // a permutation of the group's slots
                run[i] = 1;
            }
        }
    if (mixed) {
        ids[256 + 4] = 3 * 256 + 9;                    // bucket 1 (group 0) also names group 3: refused
        for (uint32_t e = 0; e < 256; ++e) run[256 + e] = 0;
    }
    std::vector<uint8_t> out(at + 8, kFill);
    const int rc = zrc4_keystream_grouped(k.c, ids.data(), declared ? bg.data() : nullptr, out.data(), off.data(),
                                          len.data(), n, nullptr);
    bool ok = rc == (mixed ? ZRC4_ERR_GROUP : ZRC4_OK);
    if (mixed)                                         // a refused bucket's spans: untouched or zero
        for (uint32_t i = 256; i < 512; ++i) {
            bool z = true, f = true;
            for (uint32_t b = 0; b < len[i]; ++b) {
                z = z && out[off[i] + b] == 0;
                f = f && out[off[i] + b] == kFill;
            }
            if (ids[i] == ZRC4_IDLE_SLOT) ok = ok && f;
            else ok = ok && (z || f);
            std::memset(&out[off[i]], kFill, len[i]);
        }
    char what[64];
    std::snprintf(what, sizeof what, "grouped%s%s", declared ? " declared" : "", mixed ? " mixed bucket" : "");
    std::vector<uint32_t> slot(ids);
    ok = spans_ok(what, k, slot, run, off, len, out) && ok;
    ok = continues_ok(what, k) && ok;
    if (!ok) std::printf("%s: rc %d -> MISMATCH\n", what, rc);
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = range_case();
    for (int d = 0; d < 2; ++d)
        for (int m = 0; m < 2; ++m) bad += grouped_case(d != 0, m != 0);
    std::printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
