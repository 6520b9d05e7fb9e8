// hooks_bcast_bench.cpp -- host-inclusive cost of one broadcast at the hooks
// interface (include/zsummerx_amd/rc4_hooks.h), no sockets, two ways in one
// process, alternating call by call:
//   copy_then_crypt  what the engine did for a loop of sendSessionData: a
//                    memcpy of the message into every session's block, then
//                    one crypt() over the blocks;
//   crypt_batch      cryptBatch() with one to-span per session, all reading
//                    the one shared message.
//   usage: hooks_bcast_bench [direct|device] [sessions] [message bytes] [reps] [rounds] [ring bytes]
// One JSON line: per variant the median of every round's calls, the median of
// those and their spread (max - min), microseconds per call.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zsummerx_amd/rc4_hooks.h"

using namespace zsummerx_amd;

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "direct";
    const uint32_t S = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 64;
    const uint32_t len = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 1024;
    const int reps = argc > 4 ? std::atoi(argv[4]) : 20;
    const int rounds = argc > 5 ? std::atoi(argv[5]) : 3;
    const uint32_t ring = argc > 6 ? (uint32_t)std::atoi(argv[6]) : 8192u;
    const uint32_t slots = (S + 255u) / 256u * 256u;
    std::unique_ptr<Rc4Hooks> h = makeDeviceRc4Hooks(0, slots, mode == "direct" ? 0u : ring);
    const size_t stride = ((size_t)len + 63) / 64 * 64 + 64;       // 64-byte aligned blocks, like the engine's
    uint8_t *pool = static_cast<uint8_t *>(h->allocBlocks((size_t)(S + 1) * stride));
    uint8_t *msg = pool + (size_t)S * stride;
    for (uint32_t i = 0; i < len; ++i) msg[i] = (uint8_t)(i * 131u + 7u);
    std::vector<uint32_t> ids(S);
    for (uint32_t i = 0; i < S; ++i) ids[i] = i;
    if (h->seed(ids.data(), S, "hooks-bcast-bench-key") != 0) return 1;
    std::vector<Rc4Span> spans(S);
    std::vector<Rc4ToSpan> to(S);
    for (uint32_t i = 0; i < S; ++i) {
        spans[i] = {i, len, pool + (size_t)i * stride};
        to[i] = {i, len, msg, pool + (size_t)i * stride};
    }
    int rc = 0;
    auto copyThenCrypt = [&] {
        for (uint32_t i = 0; i < S; ++i) std::memcpy(spans[i].data, msg, len);
        rc |= h->crypt(spans.data(), S);
    };
    auto cryptBatch = [&] { rc |= h->cryptBatch(nullptr, 0, to.data(), S, nullptr, len); };
    auto timed = [&](auto &&f) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    };
    std::vector<double> ra, rb;
    for (int r = 0; r < rounds; ++r) {
        for (int w = 0; w < 3; ++w) {
            copyThenCrypt();
            cryptBatch();
        }
        std::vector<double> a, b;
        for (int i = 0; i < reps; ++i) {
            a.push_back(timed(copyThenCrypt));
            b.push_back(timed(cryptBatch));
        }
        ra.push_back(median(a));
        rb.push_back(median(b));
    }
    if (rc) {
        std::fprintf(stderr, "hooks_bcast_bench: a hooks call failed (%d)\n", rc);
        return 1;
    }
    auto list = [](const std::vector<double> &v) {
        std::string s = "[";
        for (size_t i = 0; i < v.size(); ++i) {
            char b[32];
            std::snprintf(b, sizeof b, "%s%.2f", i ? ", " : "", v[i]);
            s += b;
        }
        return s + "]";
    };
    const double ma = median(ra), mb = median(rb);
    std::printf("{\"tool\": \"hooks_bcast_bench\", \"mode\": \"%s\", \"sessions\": %u, \"message_bytes\": %u, "
                "\"reps\": %d, \"ring\": %u, \"copy_then_crypt_round_medians_us\": %s, "
                "\"crypt_batch_round_medians_us\": %s, \"copy_then_crypt_us\": %.2f, \"crypt_batch_us\": %.2f, "
                "\"copy_then_crypt_spread_us\": %.2f, \"crypt_batch_spread_us\": %.2f, "
                "\"crypt_batch_over_copy_then_crypt\": %.3f, \"hooks\": %s}\n",
                h->name(), S, len, reps, mode == "direct" ? 0u : ring, list(ra).c_str(), list(rb).c_str(), ma, mb,
                *std::max_element(ra.begin(), ra.end()) - *std::min_element(ra.begin(), ra.end()),
                *std::max_element(rb.begin(), rb.end()) - *std::min_element(rb.begin(), rb.end()), mb / ma,
                h->stats().c_str());
    h->freeBlocks(pool);
    return 0;
}
