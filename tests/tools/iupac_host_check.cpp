// The host build of mc_iupac.h under the sanitizers, as a program of its own (no GPU, no Python):
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/tools/iupac_host_check.cpp -o iupac_host_check
//   ./iupac_host_check
// Every buffer is a heap block of exactly the contig's size, so a read or write past a contig end is an error.  The marking
// (iu_set_entry, iu_mark_strand: what mc_mark_iupac runs) is held against a letter-by-letter statement written out here, and
// the bit-plane form (iu_window_marks: what k_mark_iupac runs) against the marking, word by word.
#include "../../mcaller_amd/csrc/mc_iupac.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static uint64_t g_state = 88172645463325252ull;
static unsigned rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state >> 11); }

static bool in_set(char seq, char motif) {
    static const char *sets[] = {"AA", "CC", "GG", "TT", "RAG", "YCT", "SCG", "WAT", "KGT", "MAC", "BCGT", "DAGT", "HACT", "VACG", "NACGT"};
    for (const char *s : sets)
        if (s[0] == motif) return seq != 'M' && seq != 'N' && strchr(s + 1, seq) != nullptr;
    return false;
}

static int check(const std::string &motif, uint32_t called, size_t n, const char *alphabet) {
    mc_iupac_spec S;
    memset(&S, 0, sizeof(S));
    if (iu_set_entry(&S, 0, motif.data(), (int)motif.size(), called)) { printf("spec %s refused\n", motif.c_str()); return 1; }
    S.n_motifs = 1;
    const size_t na = strlen(alphabet), m = motif.size();
    uint8_t *upper = (uint8_t *)malloc(n ? n : 1);
    char *fwd = (char *)malloc(n ? n : 1), *rev = (char *)malloc(n ? n : 1), *want = (char *)malloc(n ? n : 1);
    for (size_t i = 0; i < n; ++i) upper[i] = (uint8_t)iu_upper((unsigned char)alphabet[rnd() % na]);
    if (n >= m && n > 0)                                      // an occurrence at the very end
        for (size_t i = 0; i < m; ++i)
            for (const char *b = "ACGT"; *b; ++b)
                if (in_set(*b, motif[i])) { upper[n - m + i] = (uint8_t)*b; break; }
    memcpy(fwd, upper, n); memcpy(rev, upper, n); memcpy(want, upper, n);
    iu_mark_strand(S.fwd, 1, upper, (int64_t)n, fwd);
    iu_mark_strand(S.rev, 1, upper, (int64_t)n, rev);
    for (size_t q = 0; q + m <= n; ++q) {
        bool hit = true;
        for (size_t i = 0; i < m && hit; ++i) hit = in_set((char)upper[q + i], motif[i]);
        if (hit)
            for (size_t j = 0; j < m; ++j)
                if ((called >> j) & 1u) want[q + j] = 'M';
    }
    int bad = memcmp(fwd, want, n) != 0;
    // the planes of the contig, and every mask word of both strands from a window of three words
    const size_t nw = (n + 31) / 32 + 2;
    std::vector<uint32_t> pl[4];
    for (auto &p : pl) p.assign(nw, 0u);
    for (size_t p = 0; p < n; ++p)
        for (int k = 0; k < 4; ++k)
            if (upper[p] == (uint8_t)"ACGT"[k]) pl[k][p / 32] |= 1u << (p % 32);
    for (size_t w = 0; w < nw && !bad; ++w) {
        iu_u128 P[4];
        for (int k = 0; k < 4; ++k)
            P[k] = (iu_u128)(w > 0 ? pl[k][w - 1] : 0u) | ((iu_u128)pl[k][w] << 32) | ((iu_u128)(w + 1 < nw ? pl[k][w + 1] : 0u) << 64);
        const uint32_t bf = (uint32_t)(iu_window_marks(&S.fwd[0], P[0], P[1], P[2], P[3]) >> 32);
        const uint32_t br = (uint32_t)(iu_window_marks(&S.rev[0], P[0], P[1], P[2], P[3]) >> 32);
        for (size_t b = 0; b < 32; ++b) {
            const size_t p = 32 * w + b;
            const bool mf = p < n && fwd[p] == 'M' && upper[p] != 'M', mr = p < n && rev[p] == 'M' && upper[p] != 'M';
            if ((((bf >> b) & 1u) != 0) != mf || (((br >> b) & 1u) != 0) != mr) bad = 2;
        }
    }
    if (bad) printf("FAILED (%d): %s called %x on %zu bases\n", bad, motif.c_str(), called, n);
    free(upper); free(fwd); free(rev); free(want);
    return bad ? 1 : 0;
}

int main() {
    struct Case { const char *motif; uint32_t called; } cases[] = {
        {"GANTC", 2u}, {"AA", 3u}, {"NAN", 2u}, {"CAAYNNNNNRTAC", 4u}, {"CRAANNNNNNNTGC", 12u}, {"A", 1u}, {"RGATCY", 16u},
        {"GANNNNNNNNNNNNNRYNNNNNNNNNNNNNTC", 2u}, {"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", 0xFFFFFFFFu}, {"BDHVKMSW", 255u}};
    int failed = 0, runs = 0;
    for (const Case &c : cases) {
        const size_t m = strlen(c.motif);
        for (size_t n : {(size_t)0, (size_t)1, m - 1, m, m + 1, (size_t)31, (size_t)32, (size_t)33, (size_t)63, (size_t)64, (size_t)65, (size_t)1000, (size_t)4097})
            for (const char *alphabet : {"ACGT", "ACGTNMacgtRY", "A", "AT"}) {
                failed += check(c.motif, c.called, n, alphabet);
                ++runs;
            }
    }
    mc_iupac_spec S;
    memset(&S, 0, sizeof(S));
    const bool refused = iu_set_entry(&S, 0, "GAXTC", 5, 2u) && iu_set_entry(&S, 0, "GATC", 4, 0u) && iu_set_entry(&S, 0, "GATC", 4, 16u) &&
                         iu_set_entry(&S, 8, "GATC", 4, 2u) && iu_set_entry(&S, 0, "", 0, 1u) &&
                         iu_set_entry(&S, 0, "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", 33, 1u);
    if (!refused) { printf("FAILED: a bad entry was accepted\n"); ++failed; }
    printf("%d runs, %d failed\n", runs, failed);
    return failed ? 1 : 0;
}
