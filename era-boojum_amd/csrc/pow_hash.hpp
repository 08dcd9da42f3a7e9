// The two hashes of the proof-of-work search (cs/implementations/pow.rs), as the search needs them:
// H(seed || nonce.to_le_bytes()) with the seed's part absorbed once on the host (the midstate) and
// only the first 32-bit digest word computed.  One __host__ __device__ definition serves the
// kernels (pow.hip), the host-side midstate and bj_pow_verify_h.  The device forms use
// v_alignbit_b32 / v_bitop3_b32; the host forms are plain C.
//
// Blake2s256 (RFC 7693, unkeyed, 32-byte digest): 64-byte blocks, the last one flagged final and
// counted with the message's length.  Keccak256: rate 136, pad10*1 with domain byte 0x01.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>

namespace bj {
namespace pow {

#define BJ_POW_HD __host__ __device__ __forceinline__

// pow.rs:67, 133: u64::from_le_bytes(digest[..8]).trailing_zeros() >= pow_bits, pow_bits <= 32
// (pow.rs:53), so the first digest word decides.  pow_bits 1..32 shift by 31..0: no shift by 32.
BJ_POW_HD uint32_t pow_mask(uint32_t pow_bits) { return pow_bits ? 0xFFFFFFFFu >> (32 - pow_bits) : 0; }
BJ_POW_HD bool pow_passes(uint32_t word0, uint32_t pow_bits) { return (word0 & pow_mask(pow_bits)) == 0; }

BJ_POW_HD uint32_t rotr32(uint32_t x, uint32_t r) {  // 0 < r < 32
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, r);
#else
    return (x >> r) | (x << (32 - r));
#endif
}
BJ_POW_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
BJ_POW_HD uint32_t chi3(uint32_t a, uint32_t b, uint32_t c) {  // a ^ (~b & c)
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xD2);
#else
    return a ^ (~b & c);
#endif
}

// ------------------------------------------------------------------ Blake2s256

constexpr uint32_t B2S_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
constexpr uint8_t B2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

#define BJ_POW_G(a, b, c, d, x, y) \
    do {                           \
        a = a + b + (x);           \
        d = rotr32(d ^ a, 16);     \
        c = c + d;                 \
        b = rotr32(b ^ c, 12);     \
        a = a + b + (y);           \
        d = rotr32(d ^ a, 8);      \
        c = c + d;                 \
        b = rotr32(b ^ c, 7);      \
    } while (0)

// RFC 7693 section 3.2 F.  A caller that reads h[0] alone leaves everything else of the last round
// dead: h[0] ^= v0 ^ v8 needs two of the four diagonal G, and of those not the last rotate of b.
BJ_POW_HD void b2s_compress(uint32_t* h, const uint32_t* m, uint64_t t, bool last) {
    uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    uint32_t v8 = B2S_IV[0], v9 = B2S_IV[1], v10 = B2S_IV[2], v11 = B2S_IV[3];
    uint32_t v12 = B2S_IV[4] ^ (uint32_t)t, v13 = B2S_IV[5] ^ (uint32_t)(t >> 32);
    uint32_t v14 = last ? ~B2S_IV[6] : B2S_IV[6], v15 = B2S_IV[7];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        BJ_POW_G(v0, v4, v8, v12, m[B2S_SIGMA[r][0]], m[B2S_SIGMA[r][1]]);
        BJ_POW_G(v1, v5, v9, v13, m[B2S_SIGMA[r][2]], m[B2S_SIGMA[r][3]]);
        BJ_POW_G(v2, v6, v10, v14, m[B2S_SIGMA[r][4]], m[B2S_SIGMA[r][5]]);
        BJ_POW_G(v3, v7, v11, v15, m[B2S_SIGMA[r][6]], m[B2S_SIGMA[r][7]]);
        BJ_POW_G(v0, v5, v10, v15, m[B2S_SIGMA[r][8]], m[B2S_SIGMA[r][9]]);
        BJ_POW_G(v1, v6, v11, v12, m[B2S_SIGMA[r][10]], m[B2S_SIGMA[r][11]]);
        BJ_POW_G(v2, v7, v8, v13, m[B2S_SIGMA[r][12]], m[B2S_SIGMA[r][13]]);
        BJ_POW_G(v3, v4, v9, v14, m[B2S_SIGMA[r][14]], m[B2S_SIGMA[r][15]]);
    }
    h[0] ^= v0 ^ v8;
    h[1] ^= v1 ^ v9;
    h[2] ^= v2 ^ v10;
    h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12;
    h[5] ^= v5 ^ v13;
    h[6] ^= v6 ^ v14;
    h[7] ^= v7 ^ v15;
}
#undef BJ_POW_G

// What a search over one seed hands to the kernel by value.  The message seed || nonce is
// seed_len + 8 bytes; its blocks that lie wholly inside the seed (none of them is the last: the
// nonce follows) are absorbed into h, and the rest is the tail: pos = seed_len mod 64 seed bytes,
// the 8 nonce bytes (left zero here) and zeros, one block, or two when pos > 56.
struct B2sMid {
    uint32_t h[8];   // chaining value after the prefix blocks
    uint64_t t[2];   // byte counter of each tail block's compression; the last used one is final
    uint32_t m[32];  // the tail's words
    uint32_t pos;    // byte offset of the nonce in the tail, 0..63
    static constexpr uint32_t FAST_POS = 40;  // the prover's seed (5 field elements): words 10, 11
    uint32_t blocks() const { return pos > 56 ? 2 : 1; }
};

inline B2sMid b2s_midstate(const uint8_t* seed, size_t seed_len) {
    B2sMid a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < 8; i++) a.h[i] = B2S_IV[i];
    a.h[0] ^= 0x01010000u ^ 32u;  // parameter block: digest 32, no key, fanout 1, depth 1
    const size_t prefix = seed_len / 64;
    uint64_t t = 0;
    for (size_t b = 0; b < prefix; b++) {
        uint32_t m[16];
        memcpy(m, seed + 64 * b, 64);  // little-endian host
        t += 64;
        b2s_compress(a.h, m, t, false);
    }
    a.pos = (uint32_t)(seed_len - 64 * prefix);
    if (a.pos) memcpy(a.m, seed + 64 * prefix, a.pos);
    if (a.pos > 56) {
        a.t[0] = t + 64;
        a.t[1] = t + a.pos + 8;
    } else {
        a.t[0] = t + a.pos + 8;
    }
    return a;
}

// The first digest word for one nonce.  FAST: pos == 40 at compile time, so the nonce is words
// 10 and 11 and words 12..15 are known zeros (their additions fold away).  Otherwise the nonce
// lands at any byte: it is shifted into three words and each tail word selects its share by a
// wave-uniform compare.
template <int BLOCKS, bool FAST>
BJ_POW_HD uint32_t b2s_word0(const B2sMid& a, uint64_t nonce) {
    const uint32_t lo = (uint32_t)nonce, hi = (uint32_t)(nonce >> 32);
    uint32_t h[8], m[16 * BLOCKS];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = a.h[i];
    if constexpr (FAST) {
        static_assert(BLOCKS == 1, "the 40-byte seed has a one-block tail");
#pragma unroll
        for (int i = 0; i < 10; i++) m[i] = a.m[i];
        m[10] = lo;
        m[11] = hi;
        m[12] = m[13] = m[14] = m[15] = 0;
    } else {
        const uint32_t w = a.pos >> 2, s = 8 * (a.pos & 3);
        const uint32_t n0 = lo << s;
        const uint32_t n1 = s ? (lo >> (32 - s)) | (hi << s) : hi;
        const uint32_t n2 = s ? hi >> (32 - s) : 0;
#pragma unroll
        for (uint32_t i = 0; i < 16 * BLOCKS; i++)
            m[i] = a.m[i] | (i == w ? n0 : 0) | (i == w + 1 ? n1 : 0) | (i == w + 2 ? n2 : 0);
    }
    if constexpr (BLOCKS == 2) {
        b2s_compress(h, m, a.t[0], false);
        b2s_compress(h, m + 16, a.t[1], true);
    } else {
        b2s_compress(h, m, a.t[0], true);
    }
    return h[0];
}

// ------------------------------------------------------------------ Keccak256

constexpr int KC_RATE = 17;  // 64-bit lanes per 136-byte block
// rho offsets of lane x + 5 y
constexpr int KC_RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};

// (hi:lo) rotated left by R (compile-time), on 32-bit halves
template <int R>
BJ_POW_HD void rotl64(uint32_t lo, uint32_t hi, uint32_t& olo, uint32_t& ohi) {
    if constexpr (R == 0) {
        olo = lo;
        ohi = hi;
    } else if constexpr (R == 32) {
        olo = hi;
        ohi = lo;
    } else if constexpr (R < 32) {
#if defined(__HIP_DEVICE_COMPILE__)
        ohi = __builtin_amdgcn_alignbit(hi, lo, 32 - R);
        olo = __builtin_amdgcn_alignbit(lo, hi, 32 - R);
#else
        ohi = (hi << R) | (lo >> (32 - R));
        olo = (lo << R) | (hi >> (32 - R));
#endif
    } else {
        rotl64<R - 32>(hi, lo, olo, ohi);
    }
}

template <int I>
BJ_POW_HD void kc_rho_pi(const uint32_t* Al, const uint32_t* Ah, uint32_t* Bl, uint32_t* Bh) {
    if constexpr (I < 25) {
        constexpr int x = I % 5, y = I / 5;
        constexpr int J = y + 5 * ((2 * x + 3 * y) % 5);
        rotl64<KC_RHO[I]>(Al[I], Ah[I], Bl[J], Bh[J]);
        kc_rho_pi<I + 1>(Al, Ah, Bl, Bh);
    }
}

BJ_POW_HD uint64_t kc_round_constant(int round) {
    constexpr uint64_t RC[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
        0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
        0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
        0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
        0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
        0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return RC[round];
}

// One round of Keccak-f[1600] (FIPS 202 section 3.2) on 32-bit lane halves, lane x + 5 y.  A
// caller that reads Al[0] alone after it leaves of chi only lane 0's low half, of rho-pi lanes 0,
// 6 and 12, and of theta those three lanes and the parities they need.
BJ_POW_HD void kc_round(uint32_t* Al, uint32_t* Ah, uint64_t rc) {
    uint32_t Cl[5], Ch[5], Rl[5], Rh[5], Bl[25], Bh[25];
#pragma unroll
    for (int x = 0; x < 5; x++) {
        Cl[x] = xor3(xor3(Al[x], Al[x + 5], Al[x + 10]), Al[x + 15], Al[x + 20]);
        Ch[x] = xor3(xor3(Ah[x], Ah[x + 5], Ah[x + 10]), Ah[x + 15], Ah[x + 20]);
    }
#pragma unroll
    for (int x = 0; x < 5; x++) rotl64<1>(Cl[x], Ch[x], Rl[x], Rh[x]);
#pragma unroll
    for (int x = 0; x < 5; x++)
#pragma unroll
        for (int y = 0; y < 5; y++) {
            Al[x + 5 * y] = xor3(Al[x + 5 * y], Cl[(x + 4) % 5], Rl[(x + 1) % 5]);
            Ah[x + 5 * y] = xor3(Ah[x + 5 * y], Ch[(x + 4) % 5], Rh[(x + 1) % 5]);
        }
    kc_rho_pi<0>(Al, Ah, Bl, Bh);
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) {
            Al[x + 5 * y] = chi3(Bl[x + 5 * y], Bl[(x + 1) % 5 + 5 * y], Bl[(x + 2) % 5 + 5 * y]);
            Ah[x + 5 * y] = chi3(Bh[x + 5 * y], Bh[(x + 1) % 5 + 5 * y], Bh[(x + 2) % 5 + 5 * y]);
        }
    Al[0] ^= (uint32_t)rc;
    Ah[0] ^= (uint32_t)(rc >> 32);
}

// rounds [from, to) as a loop (the code of one round)
BJ_POW_HD void kc_rounds(uint32_t* Al, uint32_t* Ah, int from, int to) {
#pragma unroll 1
    for (int r = from; r < to; r++) kc_round(Al, Ah, kc_round_constant(r));
}

// The midstate.  The rate blocks wholly inside the seed are absorbed and permuted on the host; the
// tail is pos = seed_len mod 136 seed bytes, the 8 nonce bytes (left zero here) and the padding
// 01 00 .. 80: one block when pos + 8 < 136, else two (the nonce straddles the blocks for pos >
// 128; at pos == 128 the second block is padding alone).  The first tail block is already XORed
// into s, the second is b2.
struct KcMid {
    uint64_t s[25];
    uint64_t b2[KC_RATE];
    uint32_t pos;  // byte offset of the nonce in the tail, 0..135
    static constexpr uint32_t FAST_POS = 40;  // the prover's seed: the nonce is lane 5
    uint32_t blocks() const { return pos >= 128 ? 2 : 1; }
};

inline KcMid kc_midstate(const uint8_t* seed, size_t seed_len) {
    KcMid a;
    memset(&a, 0, sizeof a);
    const size_t prefix = seed_len / 136;
    uint32_t Al[25] = {0}, Ah[25] = {0};
    for (size_t b = 0; b < prefix; b++) {
        uint64_t blk[KC_RATE];
        memcpy(blk, seed + 136 * b, 136);  // little-endian host
        for (int i = 0; i < KC_RATE; i++) {
            Al[i] ^= (uint32_t)blk[i];
            Ah[i] ^= (uint32_t)(blk[i] >> 32);
        }
        kc_rounds(Al, Ah, 0, 24);
    }
    a.pos = (uint32_t)(seed_len - 136 * prefix);
    uint8_t tail[2 * 136] = {0};
    if (a.pos) memcpy(tail, seed + 136 * prefix, a.pos);
    const uint32_t end = a.pos + 8, last = a.blocks() * 136 - 1;
    tail[end] ^= 0x01;
    tail[last] ^= 0x80;
    uint64_t lanes[2 * KC_RATE];
    memcpy(lanes, tail, sizeof tail);
    for (int i = 0; i < 25; i++) a.s[i] = ((uint64_t)Ah[i] << 32) | Al[i];
    for (int i = 0; i < KC_RATE; i++) {
        a.s[i] ^= lanes[i];
        a.b2[i] = lanes[KC_RATE + i];
    }
    return a;
}

// The low half of lane 0 (the first digest word) for one nonce.  Round 0 of the first permutation
// is peeled: there all lanes but the nonce's are wave-uniform, so most of it is scalar work the
// compiler hoists out of the search loop.  The last round is peeled so that its dead part goes.
template <int BLOCKS, bool FAST>
BJ_POW_HD uint32_t kc_word0(const KcMid& a, uint64_t nonce) {
    uint32_t Al[25], Ah[25];
#pragma unroll
    for (int i = 0; i < 25; i++) {
        Al[i] = (uint32_t)a.s[i];
        Ah[i] = (uint32_t)(a.s[i] >> 32);
    }
    uint64_t over = 0;  // the nonce's bytes in the second block
    if constexpr (FAST) {
        static_assert(BLOCKS == 1, "the 40-byte seed has a one-block tail");
        Al[KcMid::FAST_POS / 8] ^= (uint32_t)nonce;
        Ah[KcMid::FAST_POS / 8] ^= (uint32_t)(nonce >> 32);
    } else {
        const uint32_t q = a.pos >> 3, s = 8 * (a.pos & 7);
        const uint64_t x0 = nonce << s, x1 = s ? nonce >> (64 - s) : 0;
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)KC_RATE; i++) {
            const uint64_t x = (i == q ? x0 : 0) | (i == q + 1 ? x1 : 0);
            Al[i] ^= (uint32_t)x;
            Ah[i] ^= (uint32_t)(x >> 32);
        }
        over = q == (uint32_t)KC_RATE - 1 ? x1 : 0;
    }
    kc_round(Al, Ah, kc_round_constant(0));
    if constexpr (BLOCKS == 2) {
        kc_rounds(Al, Ah, 1, 24);
#pragma unroll
        for (int i = 0; i < KC_RATE; i++) {
            const uint64_t x = a.b2[i] ^ (i == 0 ? over : 0);
            Al[i] ^= (uint32_t)x;
            Ah[i] ^= (uint32_t)(x >> 32);
        }
        kc_rounds(Al, Ah, 0, 23);
    } else {
        kc_rounds(Al, Ah, 1, 23);
    }
    kc_round(Al, Ah, kc_round_constant(23));
    return Al[0];
}

}  // namespace pow
}  // namespace bj
