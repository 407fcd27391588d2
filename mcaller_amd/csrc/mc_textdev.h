// mc_textdev.h -- what the seven units that take whole text files through the GPU share on the device side, the twin of
// mc_textfeed.h (bed/mc_bedsum.hip with its .inc files, train/mc_trainrows.hip, merge/mc_rowmerge.hip, fastq/mc_fastqual.hip,
// compare/mc_bedcompare.hip, motifs/mc_motifscan.hip, eval/mc_evalcalls.hip).  Included by those seven units only, hence the
// unnamed namespace.
//   line_flag     a line declines its file: atomicMin of line << 8 | reason on the head's word -- the FIRST flagged line is named, and
//                 of several reasons on it the smallest, whatever the order of arrival (the host's half: decline_reason / _line)
//   ByteClass     the bytes no pipeline takes: >= 0x80; a control byte other than tab (newlines are no part of a line), 0x7f
//   KeyHash       64 bits of a key: FNV-1a over its fields' bytes, a 0xff between fields (no such byte in a text that is not
//                 declined), a finaliser, the unit's test mask (MCALLER_*_HASH_MASK=f: every key in one of 16 chains)
//   kt_claim / kt_find   an open-addressing table of keys, below
//   tabs_pack / tabs_unpack   the seven tabs of a line and its length, 16 bits each, as one uint4 per line
//   staged_lines  the text of a workgroup's 256 lines through LDS to the unit's line parser
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__device__ __forceinline__ void line_flag(unsigned long long *decline_word, long long line, int reason) {
    const unsigned long long code = ((unsigned long long)line << 8) | (unsigned)reason;
    if (code < *decline_word) atomicMin(decline_word, code);      // (the value only falls: a stale one costs an atomic, no more)
}

struct ByteClass {
    bool hi = false, ctrl = false;
    __device__ __forceinline__ void see(unsigned c) {
        hi |= c >= 0x80u;
        ctrl |= (c < 0x20u && c != '\t') || c == 0x7fu;
    }
};

struct KeyHash {
    uint64_t h = 0xcbf29ce484222325ull;
    __device__ __forceinline__ void put(char c) { h = (h ^ (uint64_t)(unsigned char)c) * 0x100000001b3ull; }
    __device__ __forceinline__ void span(const char *p, int n) { for (int i = 0; i < n; ++i) put(p[i]); }
    __device__ __forceinline__ void sep() { put((char)0xff); }
    __device__ __forceinline__ uint64_t done(uint64_t mask) const {
        uint64_t v = h;
        v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull; v ^= v >> 33;
        return v & mask;
    }
};

__device__ __forceinline__ bool same_bytes(const char *a, const char *b, int n) {
    for (int i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// ---- a table of keys: mask + 1 slots (a power of two; the host clears them: table_get), linear probing from h & mask.  A slot is
// 0 or kt_word(h, id): the tag (the high half of the key's hash) and id + 1, where the id (32 bits) names the key's bytes to the
// caller.  A slot goes from empty to taken once and its tag never changes.  same(r): is the key the caller holds the key of id r --
// r's stored hash equals h and the bytes are equal; it is asked only where the tags agree ----
struct KtHit {
    int64_t slot;            // where the key stands; -1: nowhere (kt_claim: every slot holds another key; kt_find: no such key)
    int64_t id;              // the id in that slot (kt_claim: the caller's own where it claimed the slot)
    bool claimed;
    uint64_t looked;         // slots read on the way, the last one included
};

__device__ __forceinline__ unsigned long long kt_word(uint64_t h, int64_t id) { return ((h >> 32) << 32) | (unsigned long long)(id + 1); }

// the key's slot, claimed for `id` if no slot holds the key yet (of several lanes with one key, one claims and the others find it)
template <class Same>
__device__ __forceinline__ KtHit kt_claim(unsigned long long *table, uint64_t mask, uint64_t h, int64_t id, Same same) {
    const unsigned long long mine = kt_word(h, id);
    uint64_t slot = h & mask, misses = 0;                     // misses: slots that held another key
    for (;;) {
        unsigned long long cur = table[slot];                 // (a stale "empty" is put right by the CAS)
        if (cur == 0ull) {
            cur = atomicCAS(&table[slot], 0ull, mine);
            if (cur == 0ull) return KtHit{(int64_t)slot, id, true, misses + 1};
        }
        if ((cur >> 32) == (mine >> 32)) {
            const int64_t r = (int64_t)(cur & 0xffffffffull) - 1;
            if (same(r)) return KtHit{(int64_t)slot, r, false, misses + 1};
        }
        slot = (slot + 1) & mask;
        if (++misses > mask) return KtHit{-1, -1, false, misses};      // every slot seen: the table is full (the host sizes it so that it is not)
    }
}

// the key's slot in a table that is complete (every kt_claim ran in an earlier launch)
template <class Same>
__device__ __forceinline__ KtHit kt_find(const unsigned long long *table, uint64_t mask, uint64_t h, Same same) {
    uint64_t slot = h & mask, misses = 0;
    for (;;) {
        const unsigned long long cur = table[slot];
        if (cur == 0ull) return KtHit{-1, -1, false, misses + 1};
        if ((cur >> 32) == (h >> 32)) {
            const int64_t r = (int64_t)(cur & 0xffffffffull) - 1;
            if (same(r)) return KtHit{(int64_t)slot, r, false, misses + 1};
        }
        slot = (slot + 1) & mask;
        if (++misses > mask) return KtHit{-1, -1, false, misses};
    }
}

// ---- a line's seven tabs (offsets from its start; 0 where it has fewer) and its length, 16 bits each -- a line of 65535 bytes or
// fewer -- as one uint4 per line: t0 | t1 << 16, t2 | t3 << 16, t4 | t5 << 16, t6 | len << 16 ----
struct TabSpan { uint16_t t[7], len; };

__device__ __forceinline__ uint4 tabs_pack(const int (&t)[7], int len) {
    return make_uint4((uint32_t)t[0] | ((uint32_t)t[1] << 16), (uint32_t)t[2] | ((uint32_t)t[3] << 16), (uint32_t)t[4] | ((uint32_t)t[5] << 16),
                      (uint32_t)t[6] | ((uint32_t)len << 16));
}

__device__ __forceinline__ TabSpan tabs_unpack(const uint4 r) {
    TabSpan L;
    L.t[0] = (uint16_t)r.x; L.t[1] = (uint16_t)(r.x >> 16); L.t[2] = (uint16_t)r.y; L.t[3] = (uint16_t)(r.y >> 16);
    L.t[4] = (uint16_t)r.z; L.t[5] = (uint16_t)(r.z >> 16); L.t[6] = (uint16_t)r.w; L.len = (uint16_t)(r.w >> 16);
    return L;
}

// ---- The text of the lines [256 * blockIdx.x, + 256) of a workgroup of 256 threads, staged in LDS by 16-byte loads from the aligned
// address at or below its first byte (the text buffer is padded: whole 16-byte groups are readable; the launch gives STAGE + 16
// bytes of dynamic LDS).  Thread k then calls parse(t, adj, line) for its line, where t[x - adj] is byte x of the text: the staged
// piece, or -- a piece over STAGE bytes, very long lines -- the text itself with adj = 0.  Two calls, so that each is compiled
// for one address space.  -> whether the workgroup read in place ----
template <int STAGE, class Parse>
__device__ __forceinline__ bool staged_lines(const char *text, int64_t n_bytes, const long long *line_start, int64_t n_lines, int64_t n_nl, Parse parse) {
    extern __shared__ __attribute__((aligned(16))) char s_text[];
    const int64_t l0 = (int64_t)blockIdx.x * 256;
    const int64_t l1 = min(l0 + 256, n_lines);
    const int64_t g0 = line_start[l0], g1 = l1 <= n_nl ? (int64_t)line_start[l1] : n_bytes;
    const int64_t a0 = g0 & ~(int64_t)15;
    const int64_t li = l0 + threadIdx.x;
    if (g1 - a0 <= STAGE) {
        for (int64_t i = (int64_t)threadIdx.x * 16; i < g1 - a0; i += 256 * 16)
            *reinterpret_cast<uint4 *>(s_text + i) = *reinterpret_cast<const uint4 *>(text + a0 + i);
        __syncthreads();
        if (li < l1) parse((const char *)s_text, a0, li);
        return false;
    }
    if (li < l1) parse(text, (int64_t)0, li);
    return true;
}

}  // namespace
