// gol_ckpt_file.h — the checkpoint file of a board: its
// 64-byte header and the checks a reader makes before it trusts one.  Plain
// C++17 with no device header, so that golhip_checkpoint_info, the host mirror
// and a stand-alone test program include the same code.
//
// The file, little-endian, exactly 64 + 4 * height * Ww bytes, Ww = ceil(width / 32):
//   q0  the 8 bytes "GOLCKPT" 0x01
//   q1  version (1) | header bytes (64) << 32
//   q2  width | height << 32
//   q3  turn (int64)
//   q4  alive cells of the whole board
//   q5  golhip_board_hash of the whole board
//   q6  Ww | 0 << 32
//   q7  sum over i = 0..6 of splitmix64(q_i + i), mod 2^64
// then the board's canonical bit words, row-major, padding bits zero.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

namespace golckpt {

constexpr uint64_t kHeaderBytes = 64;
constexpr uint32_t kVersion = 1;
constexpr unsigned char kMagic[8] = {'G', 'O', 'L', 'C', 'K', 'P', 'T', 0x01};

struct Header {
    int32_t width = 0, height = 0;
    int64_t turn = 0;
    uint64_t alive = 0, hash = 0;
    uint32_t Ww = 0;
    uint64_t file_bytes() const { return kHeaderBytes + 4ull * (uint64_t)height * Ww; }
};

inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline uint64_t get_u64(const unsigned char *p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return v;
}
inline void put_u64(unsigned char *p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (8 * i));
}
inline uint64_t header_check(const uint64_t q[7]) {
    uint64_t s = 0;
    for (uint64_t i = 0; i < 7; ++i) s += splitmix64(q[i] + i);
    return s;
}

inline void encode(const Header &h, unsigned char out[kHeaderBytes]) {
    uint64_t q[8];
    q[0] = get_u64(kMagic);
    q[1] = (uint64_t)kVersion | (kHeaderBytes << 32);
    q[2] = (uint64_t)(uint32_t)h.width | ((uint64_t)(uint32_t)h.height << 32);
    q[3] = (uint64_t)h.turn;
    q[4] = h.alive;
    q[5] = h.hash;
    q[6] = (uint64_t)h.Ww;
    q[7] = header_check(q);
    for (int i = 0; i < 8; ++i) put_u64(out + 8 * i, q[i]);
}

// The checks of a header of `have` bytes read from a file of `file_size`
// bytes, in this order: size (a whole header), magic, version, header check,
// geometry, size (header + payload).  Returns true and fills *h, or false
// with the failed check named in *why.
inline bool decode(const unsigned char *bytes, uint64_t have, uint64_t file_size, Header *h, std::string *why) {
    if (have < kHeaderBytes || file_size < kHeaderBytes) {
        *why = "file size: " + std::to_string(file_size) + " bytes, less than the 64-byte header";
        return false;
    }
    uint64_t q[8];
    for (int i = 0; i < 8; ++i) q[i] = get_u64(bytes + 8 * i);
    if (q[0] != get_u64(kMagic)) {
        *why = "magic: not a GOLCKPT file";
        return false;
    }
    if ((uint32_t)q[1] != kVersion || (q[1] >> 32) != kHeaderBytes) {
        *why = "version: " + std::to_string((uint32_t)q[1]) + " with a header of " + std::to_string(q[1] >> 32) +
               " bytes (this reader: version 1, 64 bytes)";
        return false;
    }
    if (q[7] != header_check(q)) {
        *why = "header check: the header's fields do not sum to its check word";
        return false;
    }
    const uint64_t w = q[2] & 0xFFFFFFFFull, ht = q[2] >> 32;
    if (w == 0 || ht == 0 || w > 0x7FFFFFFFull || ht > 0x7FFFFFFFull || (q[6] >> 32) != 0 ||
        (q[6] & 0xFFFFFFFFull) != (w + 31) / 32 || (int64_t)q[3] < 0) {
        *why = "header check: impossible geometry or turn (" + std::to_string(w) + " x " + std::to_string(ht) + ", " +
               std::to_string(q[6]) + " words a row, turn " + std::to_string((int64_t)q[3]) + ")";
        return false;
    }
    h->width = (int32_t)w;
    h->height = (int32_t)ht;
    h->turn = (int64_t)q[3];
    h->alive = q[4];
    h->hash = q[5];
    h->Ww = (uint32_t)q[6];
    if (file_size != h->file_bytes()) {
        *why = "file size: " + std::to_string(file_size) + " bytes, the header's board needs " +
               std::to_string(h->file_bytes());
        return false;
    }
    return true;
}

// Header and size of the file at `path`.  0: fine; 1: the file cannot be
// opened or read (*why has the reason); 2: it is damaged (*why names the check).
inline int read_info(const char *path, Header *h, std::string *why) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) {
        *why = std::string("open ") + path + ": cannot open";
        return 1;
    }
    unsigned char buf[kHeaderBytes];
    const size_t got = std::fread(buf, 1, sizeof buf, f);
    long long size = -1;
    if (std::fseek(f, 0, SEEK_END) == 0) size = (long long)std::ftell(f);
    std::fclose(f);
    if (size < 0) {
        *why = std::string("size of ") + path + ": cannot seek";
        return 1;
    }
    return decode(buf, got, (uint64_t)size, h, why) ? 0 : 2;
}

}  // namespace golckpt
