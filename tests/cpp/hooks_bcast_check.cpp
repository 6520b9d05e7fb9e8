// hooks_bcast_check.cpp -- TEST INFRASTRUCTURE ONLY.
// Drives Rc4Hooks::cryptBatch (include/zsummerx_amd/rc4_hooks.h) the way the
// engine's broadcast does -- S sessions of a read and a write slot; per round
// random in-place spans on both, and out-of-place spans ("to") on the write
// slots whose sources are a few shared messages, whole or a prefix, congruent
// mod 16 with the destination or not -- and checks the WHOLE pool against the
// oracle RC4 (oracle/rc4_oracle.c) after every call: the destinations, the
// sources unchanged, and every byte no span names.  A write slot is idle, in
// place only, a to-span at the block start, staged bytes with the to-span
// directly behind them (the engine's reply-then-broadcast), or the two apart.
// Sessions are reseeded on the way; plain crypt() calls between the rounds and
// at the end check the states a cryptBatch leaves.
//   usage: hooks_bcast_check [device|direct|base] [sessions] [rounds] [seed] [ring bytes]
// base: the interface's own cryptBatch over hooks that have only crypt() (the
// oracle).  A ring below the message size forces ring wrap, partial coverage
// and device tails of both lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "zrc4.h"
#include "zsummerx_amd/rc4_hooks.h"
extern "C" {
#include "rc4_oracle.h"
}

using namespace zsummerx_amd;

namespace {

// Hooks with nothing but crypt(): cryptBatch is the base class's.
class OracleHooks final : public Rc4Hooks {
public:
    explicit OracleHooks(uint32_t slots) : st_(slots) {}
    const char *name() const override { return "oracle"; }
    uint32_t capacity() const override { return (uint32_t)st_.size(); }
    void *allocBlocks(size_t bytes) override { return std::aligned_alloc(64, (bytes + 63) / 64 * 64); }
    void freeBlocks(void *p) override { std::free(p); }
    int seed(const uint32_t *slots, uint32_t n, const std::string &key) override
    {
        for (uint32_t i = 0; i < n; ++i)
            oracle_make_sbox(&st_[slots[i]], reinterpret_cast<const uint8_t *>(key.data()), key.size());
        return ZRC4_OK;
    }
    int crypt(const Rc4Span *s, uint32_t n) override
    {
        for (uint32_t i = 0; i < n; ++i) oracle_encryption(&st_[s[i].slot], s[i].data, s[i].len);
        return ZRC4_OK;
    }

private:
    std::vector<oracle_rc4_state> st_;
};

constexpr uint32_t kData = 2048;          // bytes of a slot's block
constexpr size_t kBlk = kData + 64;       // block stride (64-byte aligned starts, a guard gap between blocks)
constexpr uint32_t kMsgs = 4;

}  // namespace

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "device";
    const uint32_t S = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 64;
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 40;
    std::mt19937 rng(argc > 4 ? std::atoi(argv[4]) : 1);
    const uint32_t slots = 2 * S;
    const uint32_t ring = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 32768u;
    std::unique_ptr<Rc4Hooks> h;
    if (mode == "base") h.reset(new OracleHooks(slots));
    else h = makeDeviceRc4Hooks(0, slots, mode == "direct" ? 0u : ring);

    // pool: 64 guard bytes, one block per slot, then the shared messages
    const size_t poolBytes = 64 + (size_t)(slots + kMsgs) * kBlk;
    uint8_t *pool = static_cast<uint8_t *>(h->allocBlocks(poolBytes));
    auto block = [&](uint32_t i) { return pool + 64 + (size_t)i * kBlk; };
    std::vector<uint8_t> want(poolBytes, 0xA5);
    std::memset(pool, 0xA5, poolBytes);
    auto mirror = [&](const uint8_t *p) { return want.data() + (p - pool); };

    std::vector<oracle_rc4_state> ref(slots);
    auto seedSession = [&](uint32_t s) {
        std::string k;
        const int kl = 1 + (int)(rng() % 30);
        for (int i = 0; i < kl; ++i) k.push_back((char)(rng() & 255));
        const uint32_t two[2] = {2 * s, 2 * s + 1};
        h->seed(two, 2, k);
        oracle_make_sbox(&ref[2 * s], reinterpret_cast<const uint8_t *>(k.data()), k.size());
        oracle_make_sbox(&ref[2 * s + 1], reinterpret_cast<const uint8_t *>(k.data()), k.size());
    };
    for (uint32_t s = 0; s < S; ++s) seedSession(s);

    auto fail = [&](const char *what, int r, int rc) {
        std::printf("{\"ok\": false, \"mode\": \"%s\", \"what\": \"%s\", \"round\": %d, \"rc\": %d}\n", mode.c_str(),
                    what, r, rc);
        return 1;
    };
    // the whole pool against its mirror: '' or the first difference
    auto compare = [&](const char *what, int r) {
        if (!std::memcmp(pool, want.data(), poolBytes)) return 0;
        size_t at = 0;
        while (pool[at] == want[at]) ++at;
        const long blk = at < 64 ? -1 : (long)((at - 64) / kBlk);
        std::printf("{\"ok\": false, \"mode\": \"%s\", \"what\": \"%s\", \"round\": %d, \"pool_byte\": %zu, "
                    "\"block\": %ld, \"block_byte\": %zu, \"got\": %u, \"want\": %u}\n",
                    mode.c_str(), what, r, at, blk, at < 64 ? at : (at - 64) % kBlk, pool[at], want[at]);
        return 2;
    };
    // fresh plaintext in [d, d + len) of both pool and mirror
    auto fill = [&](uint8_t *d, uint32_t len) {
        for (uint32_t i = 0; i < len; ++i) d[i] = (uint8_t)rng();
        std::memcpy(mirror(d), d, len);
    };
    auto randLen = [&](uint32_t most) {
        const uint32_t pick = rng() % 10;
        const uint32_t len = pick < 3 ? 1 + rng() % 17 : pick < 6 ? 1 + rng() % 300 : 1 + rng() % kData;
        return len < most ? len : most;
    };

    unsigned long long bytes = 0, toBytes = 0, toSpans = 0, both = 0, apart = 0, skew = 0;
    std::vector<Rc4Span> spans;
    std::vector<Rc4ToSpan> to;
    for (int r = 0; r < rounds; ++r) {
        if (r && r % 7 == 0) seedSession(rng() % S);              // reconnect
        // the round's messages, each at a start of any alignment
        uint32_t mlen[kMsgs], mat[kMsgs];
        for (uint32_t m = 0; m < kMsgs; ++m) {
            mlen[m] = m == 0 ? kData - 15 : randLen(kData - 15);
            mat[m] = rng() % 4 ? 0 : rng() % 16;
            fill(block(slots + m) + mat[m], mlen[m]);
        }
        spans.clear();
        to.clear();
        for (uint32_t sl = 0; sl < slots; ++sl) {
            uint8_t *b = block(sl);
            const uint32_t kind = sl % 2 == 0 ? (rng() % 3 ? 1u : 0u) : rng() % 5;   // read slots: idle or in place
            if (kind == 0) continue;
            uint32_t staged = 0;
            if (kind == 1 || kind >= 3) {                         // in place, from any start
                const uint32_t start = kind == 1 ? rng() % 64 : 0;
                const uint32_t len = randLen(kind == 1 ? kData - start : kData / 2);
                fill(b + start, len);
                oracle_encryption(&ref[sl], mirror(b + start), len);
                spans.push_back({sl, len, b + start});
                bytes += len;
                staged = start + len;
            }
            if (kind >= 2) {
                // 2: at the block start; 3: directly behind the staged bytes; 4: apart from them
                const uint32_t at = kind == 2 ? 0 : kind == 3 ? staged : staged + 1 + rng() % 40;
                const uint32_t m = rng() % kMsgs;
                uint32_t len = rng() % 3 ? mlen[m] : 1 + rng() % mlen[m];    // the message, or a prefix of it
                if (len > kData - at) len = kData - at;
                const uint8_t *src = block(slots + m) + mat[m];
                uint8_t *dst = b + at;
                std::memcpy(mirror(dst), src, len);
                oracle_encryption(&ref[sl], mirror(dst), len);
                to.push_back({sl, len, src, dst});
                toBytes += len;
                ++toSpans;
                both += kind >= 3;
                apart += kind == 4;
                skew += ((uintptr_t)src - (uintptr_t)dst) % 16 != 0;
            }
        }
        int rc = h->cryptBatch(spans.data(), (uint32_t)spans.size(), to.data(), (uint32_t)to.size(), nullptr, kData);
        if (rc) return fail("cryptBatch", r, rc);
        if (compare("cryptBatch", r)) return 2;
        if (r % 3 == 2) {
            // a plain crypt() behind it, over every slot: the states it left
            spans.clear();
            for (uint32_t sl = 0; sl < slots; ++sl) {
                const uint32_t len = 1 + rng() % 96;
                uint8_t *d = block(sl) + rng() % 128;
                fill(d, len);
                oracle_encryption(&ref[sl], mirror(d), len);
                spans.push_back({sl, len, d});
                bytes += len;
            }
            if ((rc = h->crypt(spans.data(), (uint32_t)spans.size())) != 0) return fail("crypt", r, rc);
            if (compare("crypt", r)) return 2;
        }
    }
    // a slot twice among the to-spans is refused by the device hooks, nothing touched
    if (mode != "base") {
        const uint8_t *src = block(slots);
        const Rc4ToSpan dup[2] = {{1, 16, src, block(1)}, {1, 16, src, block(1) + 32}};
        const int rc = h->cryptBatch(nullptr, 0, dup, 2, nullptr, kData);
        if (rc != ZRC4_ERR_INVALID_ARG) return fail("duplicate", rounds, rc);
        if (compare("duplicate", rounds)) return 2;
    }
    std::printf("{\"ok\": true, \"mode\": \"%s\", \"sessions\": %u, \"rounds\": %d, \"bytes\": %llu, "
                "\"to_spans\": %llu, \"to_bytes\": %llu, \"slot_in_both\": %llu, \"apart\": %llu, "
                "\"non_congruent\": %llu, \"hooks\": %s}\n",
                mode.c_str(), S, rounds, bytes, toSpans, toBytes, both, apart, skew, h->stats().c_str());
    h->freeBlocks(pool);
    return 0;
}
