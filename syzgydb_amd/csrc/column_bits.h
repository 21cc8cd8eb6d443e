// column_bits.h -- the host-only bit arithmetic of the resident columns (scan_column.cpp): a caller's present bits are
// shifted into place here, so this is the one part that indexes a caller's buffer by arithmetic of its own.  No HIP in
// here: tests/cpp/test_column_bits.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>

namespace szgi {

// n bits of src from bit src_off (src null: ones) to dst from bit dst_off; the other bits of dst stay.  Reads the words
// of src that hold bits [src_off, src_off + n) and no others; writes the words of dst that hold [dst_off, dst_off + n).
inline void copy_bits(uint64_t *dst, uint64_t dst_off, const uint64_t *src, uint64_t src_off, uint64_t n)
{
    while (n) {
        const unsigned db = (unsigned)(dst_off & 63);
        const uint64_t take = std::min<uint64_t>(n, 64 - db);
        uint64_t bits = ~0ull;
        if (src) {
            const unsigned sb = (unsigned)(src_off & 63);
            bits = src[src_off >> 6] >> sb;
            if (sb && take > 64 - sb) bits |= src[(src_off >> 6) + 1] << (64 - sb);
        }
        const uint64_t field = (take == 64 ? ~0ull : ((1ull << take) - 1ull)) << db;
        uint64_t &w = dst[dst_off >> 6];
        w = (w & ~field) | ((bits << db) & field);
        dst_off += take, src_off += take, n -= take;
    }
}

}  // namespace szgi
