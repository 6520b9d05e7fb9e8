// emu_zrc4_keystream.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The write-only keystream calls (include/zrc4.h: zrc4_keystream_range,
// zrc4_keystream_grouped) over the public emulated zrc4 C-ABI of
// emu_zrc4_hip.cpp, with which it is linked: the span of every entry that is
// not skipped is zeroed (whatever it held is never read), then the emulated
// crypt call runs over it (0 ^ k = k).  Skipped entries -- len 0, an idle id,
// an id >= capacity -- keep their bytes; a refused bucket's spans end up zero,
// one of the two outcomes the header allows.
#include <cstring>
#include <vector>

#include "zrc4.h"

extern "C" {

int zrc4_keystream_range(zrc4_ctx *c, uint32_t first_slot, uint8_t *out, const uint64_t *off, const uint32_t *len,
                         uint32_t n, void *s)
{
    if (!c || (n && (!out || !off || !len))) return ZRC4_ERR_INVALID_ARG;
    if ((uint64_t)first_slot + n > zrc4_capacity(c)) return ZRC4_ERR_SLOT_RANGE;
    // (the emulated zrc4_crypt_range is zrc4_crypt with explicit ids)
    std::vector<uint32_t> ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        ids[i] = first_slot + i;
        if (len[i]) std::memset(out + off[i], 0, len[i]);
    }
    return zrc4_crypt(c, ids.data(), out, off, len, n, s);
}

int zrc4_keystream_grouped(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, uint8_t *out,
                           const uint64_t *off, const uint32_t *len, uint32_t n, void *s)
{
    if (!c || (n && (!ids || !out || !off || !len))) return ZRC4_ERR_INVALID_ARG;
    const uint32_t cap = zrc4_capacity(c);
    if (bucket_group)
        for (uint32_t b = 0; b < (n + 255u) / 256u; ++b)
            if (bucket_group[b] >= cap / 256u && bucket_group[b] != ZRC4_IDLE_SLOT) return ZRC4_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (len[i] && ids[i] < cap) std::memset(out + off[i], 0, len[i]);     // (ZRC4_IDLE_SLOT is >= cap)
    return bucket_group ? zrc4_crypt_grouped_declared(c, ids, bucket_group, out, off, len, n, nullptr, s)
                        : zrc4_crypt_grouped(c, ids, out, off, len, n, s);
}

}  // extern "C"
