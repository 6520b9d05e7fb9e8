// emu_zrc4_crypt_to.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The out-of-place grouped crypt call (include/zrc4.h: zrc4_crypt_to_grouped)
// over the public emulated zrc4 C-ABI of emu_zrc4_hip.cpp, with which it is
// linked: the source span of every entry that is not skipped is copied into
// its destination span (an entry whose two addresses are identical is left
// alone), then the emulated in-place crypt call runs over the destinations --
// the two-launch form the header describes.  Sources are never written and a
// destination is never read before it is written.  Skipped entries -- len 0,
// an idle id, an id >= capacity -- keep their destination bytes; a refused
// bucket's spans end up a plain copy of the source, one of the two outcomes
// the header allows.
#include <cstring>

#include "zrc4.h"

extern "C" {

int zrc4_crypt_to_grouped(zrc4_ctx *c, const uint32_t *ids, const uint32_t *bucket_group, const uint8_t *src,
                          const uint64_t *src_off, uint8_t *dst, const uint64_t *dst_off, const uint32_t *len,
                          uint32_t n, void *s)
{
    if (!c || (n && (!ids || !src || !src_off || !dst || !dst_off || !len))) return ZRC4_ERR_INVALID_ARG;
    const uint32_t cap = zrc4_capacity(c);
    if (bucket_group)
        for (uint32_t b = 0; b < (n + 255u) / 256u; ++b)
            if (bucket_group[b] >= cap / 256u && bucket_group[b] != ZRC4_IDLE_SLOT) return ZRC4_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        if (!len[i] || ids[i] >= cap) continue;                    // (ZRC4_IDLE_SLOT is >= cap)
        const uint8_t *from = src + src_off[i];
        uint8_t *to = dst + dst_off[i];
        if (from != to) std::memcpy(to, from, len[i]);
    }
    return bucket_group ? zrc4_crypt_grouped_declared(c, ids, bucket_group, dst, dst_off, len, n, nullptr, s)
                        : zrc4_crypt_grouped(c, ids, dst, dst_off, len, n, s);
}

}  // extern "C"
