// mc_motifiupac.inc -- find_motifs --iupac behind km_count (part of mc_motifscan.hip; the definition: mcaller_amd/find_motifs.py):
// from "which concrete entries are methylated" to "which degenerate patterns are", with no second pass over the genome.
//
// A table of k X has n = k - 1 free X (the called one is --base).  A pattern is n base-15 digits, digit = mask - 1 over A = 1, C = 2,
// G = 4, T = 8, the first free X the highest digit -- so the order of the indices is the order of the masks from left to right.
// Its purity flag is ONE BYTE at lattice[T.lat + index]: 15^n bytes a table, 171 MB for 8 X; every lattice of the call is resident
// until the parent test is done (the need is counted against free device memory before anything is allocated).  Bytes, not packed
// bits: 15^s is odd, so a packed row would begin at a different bit phase for every value of the higher digits, and the neighbour
// and parent reads take single flags at strides of 15^d anyway.
//   ki_good      a lane per concrete entry: nCovered >= 1 and one IEEE fp64 division against min_fraction -> a byte
//   ki_widen     the AND transform, a launch per free X and table, the LOWEST digit first: the pass s reads [hi][4][lo] and writes
//                [hi][15][lo], lo = 15^s, hi = 4^(n - 1 - s); an output byte ANDs the 1 to 4 inputs of its mask, lo bytes apart,
//                and a lane makes four of them and stores one word (a fifth less time than a byte a lane).  All passes run in global memory (no LDS stage for the low digits: the first passes are the small ones).
//                A pass reads 4^(n - s) 15^s bytes and writes 4^(n - 1 - s) 15^(s + 1); the passes before the last go through two
//                scratch blocks of 4 x 15^(n - 1) bytes, the last one writes the lattice: 45.6 MB read, 171 MB written for 8 X,
//                1.36 x 15^n bytes moved by all passes together.  No size is a multiple of a wave: every lane is guarded by its
//                index, no grid is rounded to anything but whole workgroups.  A table's lattice begins at a multiple of 16 bytes.
//   ki_maximal   a lane per pattern: pure, and none of the at most 3 n patterns with one more letter at one X is (reads at stride
//                15^d; an impure pattern costs its one byte).  Run twice per table: to count (n_pure, n_maximal), then -- the
//                list has its size -- to put (table, index) into it.  Slots by atomicAdd: the order of the list decides nothing
//   ki_sums      a wave per maximal pattern (they are rare): the integer sums of its members' three counters, lanes over the
//                product of the sets, __shfl_xor.  No floating-point atomic, no result that depends on an order of arrival
//   ki_pick      a lane per maximal pattern: both thresholds (the division kept, as the definition says), then for every parent
//                table the flag of the pattern restricted to the parent's X, its index built from the row's own digits
//   kp_scan / ki_gather   the survivors numbered in list order and copied out; the host sorts them by the integer keys of the
//                definition and prints them with mc_rowtext.h

struct MiHead {                              // device-side result block
    unsigned long long n_good, n_pure, n_maximal, n_selected, cursor;
    long long n_rows;
};

struct MiPat { int32_t table; uint32_t index, nG, nC, nM; };

struct MiArgs {
    const MsTable *tables;
    const MsParent *parents;
    const unsigned int *nG, *nC, *nM;        // nC: nG where there is no control
    int64_t n_entries;
    long long min_sites;
    double min_fraction;
    int32_t keep_all, pad;
    uint8_t *good, *lattice;
    MiHead *head;
    MiPat *pats, *rows;
    int64_t n_pats;
    long long *flag, *place;
};

__host__ __device__ inline uint32_t mi_pow15(int n) {
    uint32_t v = 1;
    for (int i = 0; i < n; ++i) v *= 15u;
    return v;
}

__global__ __launch_bounds__(256) void ki_good(MiArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool good = false;
    if (e < A.n_entries) {
        const unsigned int nC = A.nC[e];
        good = nC >= 1u && (double)A.nM[e] / (double)nC >= A.min_fraction;
        A.good[e] = good ? 1 : 0;
    }
    const uint64_t any = __ballot(good);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&A.head->n_good, (unsigned long long)__popcll(any));
}

// in: [hi][4][lo], out: [hi][15][lo]; n_out = hi * 15 * lo < 2^32.  A lane makes four consecutive output bytes and stores them as one
// word (out is 4-byte aligned: the scratch blocks are allocations, the lattices begin at multiples of 16); the last lane of a launch
// may hold fewer than four and stores them one by one
__global__ __launch_bounds__(256) void ki_widen(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t lo, uint32_t n_out) {
    const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (first >= n_out) return;
    const uint32_t i = (uint32_t)first;
    uint32_t l = i % lo, m = i / lo % 15u, h = i / lo / 15u, word = 0;
    const int n = (int)min(4u, n_out - i);
    for (int b = 0; b < n; ++b) {
        const uint8_t *p = in + ((size_t)h * 4) * lo + l;
        const uint32_t mask = m + 1;
        uint32_t v = 1;
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if ((mask >> a) & 1u) v &= p[(size_t)a * lo];
        word |= (v & 1u) << (8 * b);
        if (++l == lo) { l = 0; if (++m == 15u) { m = 0; ++h; } }
    }
    if (n == 4) *reinterpret_cast<uint32_t *>(out + i) = word;
    else
        for (int b = 0; b < n; ++b) out[i + b] = (uint8_t)(word >> (8 * b));
}

// is the pure pattern `i` of a lattice of n digits maximal: no pattern with one more letter at one X is pure
__device__ __forceinline__ bool mi_is_maximal(const uint8_t *lat, uint32_t i, int n) {
    uint32_t stride = 1, rest = i;
    for (int d = 0; d < n; ++d) {
        const uint32_t mask = rest % 15u + 1;
        rest /= 15u;
        for (int a = 0; a < 4; ++a)
            if (!((mask >> a) & 1u) && lat[i + (1u << a) * stride]) return false;       // (mask | bit) - mask = bit
        stride *= 15u;
    }
    return true;
}

template <bool GATHER>
__global__ __launch_bounds__(256) void ki_maximal(MiArgs A, int ti, uint32_t n_lat) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const MsTable &T = A.tables[ti];
    const uint8_t *lat = A.lattice + T.lat;
    const bool pure = g < n_lat && lat[g];
    const bool maximal = pure && mi_is_maximal(lat, (uint32_t)g, T.k - 1);
    if (GATHER) {
        if (!maximal) return;
        const unsigned long long at = atomicAdd(&A.head->cursor, 1ull);
        if ((int64_t)at < A.n_pats) A.pats[at] = MiPat{ti, (uint32_t)g, 0u, 0u, 0u};      // (always: the first run counted them)
    } else {
        const uint64_t np = __ballot(pure), nm = __ballot(maximal);
        if ((threadIdx.x & 63) == 0 && np) {
            atomicAdd(&A.head->n_pure, (unsigned long long)__popcll(np));
            if (nm) atomicAdd(&A.head->n_maximal, (unsigned long long)__popcll(nm));
        }
    }
}

__global__ __launch_bounds__(256) void ki_sums(MiArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= A.n_pats) return;                                         // (a whole wave leaves)
    const int lane = threadIdx.x & 63;
    const MiPat P = A.pats[p];
    const MsTable &T = A.tables[P.table];
    const int n = T.k - 1;
    uint32_t mask[8], rest = P.index, members = 1;
    for (int d = n - 1; d >= 0; --d) {                                 // mask[d]: of free X d, left to right
        mask[d] = rest % 15u + 1;
        rest /= 15u;
        members *= (uint32_t)__popc(mask[d]);
    }
    unsigned long long sG = 0, sC = 0, sM = 0;
    for (uint32_t m = lane; m < members; m += 64) {
        uint32_t key = 0, r = m;
        for (int d = n - 1; d >= 0; --d) {                             // the last free X is the key's lowest letter
            const uint32_t c = (uint32_t)__popc(mask[d]);
            uint32_t pick = r % c, bits = mask[d];
            r /= c;
            for (; pick; --pick) bits &= bits - 1;                     // drop the `pick` lowest letters of the set
            key |= (uint32_t)(__ffs((int)bits) - 1) << (2 * (n - 1 - d));
        }
        if (key >= T.entries) continue;                                // (cannot be: n letters of two bits)
        sG += A.nG[T.off + key]; sC += A.nC[T.off + key]; sM += A.nM[T.off + key];
    }
    for (int o = 32; o > 0; o >>= 1) {
        sG += __shfl_xor(sG, o); sC += __shfl_xor(sC, o); sM += __shfl_xor(sM, o);
    }
    if (lane == 0) { A.pats[p].nG = (uint32_t)sG; A.pats[p].nC = (uint32_t)sC; A.pats[p].nM = (uint32_t)sM; }
}

__global__ __launch_bounds__(256) void ki_pick(MiArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool sel = false, keep = false;
    if (p < A.n_pats) {
        const MiPat P = A.pats[p];
        sel = keep = (long long)P.nM >= A.min_sites && (double)P.nM / (double)P.nC >= A.min_fraction;
        if (sel && !A.keep_all) {
            const MsTable &T = A.tables[P.table];
            uint32_t digit[8], rest = P.index;                         // digit[q]: of the child's X q (the called one: unused)
            for (int q = T.k - 1; q >= 0; --q) {
                if (q == T.j) { digit[q] = 0; continue; }
                digit[q] = rest % 15u;
                rest /= 15u;
            }
            for (int u = T.parent_lo; u < T.parent_hi && keep; ++u) {
                const MsParent &R = A.parents[u];
                const MsTable &U = A.tables[R.table];
                uint32_t at = 0;
                for (int i = 0; i < U.k; ++i)
                    if (i != U.j) at = at * 15u + digit[R.from[i] & 7];
                if (at < mi_pow15(U.k - 1) && A.lattice[U.lat + at]) keep = false;
            }
        }
        A.flag[p] = keep ? 1 : 0;
    }
    const uint64_t any = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(&A.head->n_selected, (unsigned long long)__popcll(any));
}

__global__ __launch_bounds__(256) void ki_gather(MiArgs A) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pats || !A.flag[p]) return;
    A.rows[A.place[p]] = A.pats[p];
}

// what --iupac needs on the device beside the plain mode's: the good flags, every lattice and the two scratch blocks of the
// transform; the tables' places in the lattice block
inline size_t mi_need(std::vector<MsTable> &tables, size_t *scratch) {
    size_t lat = 0, entries = 0;
    *scratch = 0;
    for (MsTable &T : tables) {
        T.lat = lat;
        lat += ((size_t)mi_pow15(T.k - 1) + 15) & ~(size_t)15;
        entries += T.entries;
        if (T.k > 2) *scratch = std::max(*scratch, (size_t)4 * mi_pow15(T.k - 2));
    }
    return lat + 2 * *scratch + entries;
}

struct MiState {                             // what a call keeps on the device behind km_count, allocated once
    MiArgs M = {};
    uint8_t *tmp[2] = {nullptr, nullptr};
    int64_t cap_pats = 0;
};

// A.nG / nC / nM hold the counts of every table; `tables` carry their places in the lattice block
int mi_setup(Pool &pool, const MsArgs &A, const std::vector<MsTable> &tables, size_t scratch, MiState &mi) {
    MiArgs &M = mi.M;
    M.tables = A.tables; M.parents = A.parents;
    M.nG = A.nG; M.nC = A.has_control ? A.nC : A.nG; M.nM = A.nM;
    M.n_entries = A.n_entries; M.min_sites = A.min_sites; M.min_fraction = A.min_fraction; M.keep_all = A.keep_all;
    const size_t n_lat = tables.back().lat + mi_pow15(tables.back().k - 1);
    if (pool.get(&M.good, (size_t)A.n_entries) || pool.get(&M.lattice, n_lat) || pool.get(&mi.tmp[0], scratch + 1) ||
        pool.get(&mi.tmp[1], scratch + 1) || pool.get(&M.head, 1))
        return -10;
    return 0;
}

// The tables are counted -> the rows of the definition in its order, in structured form.  again (--iterative, rounds 2 on): the
// stats keep round 1's figures; the flags, the lattices and the head are made anew every round
int mi_rows(mc_ctx *c, Pool &pool, MiState &mi, const std::vector<MsTable> &tables, bool again, std::vector<MiPat> &rows,
            std::chrono::steady_clock::time_point *t_d2h, int32_t *status) {
    mc_motif_stats &S = c->motif.stats;
    mc_motif_iupac_stats &I = c->motif.iupac_stats;
    hipStream_t st = c->stream;
    MiArgs &M = mi.M;
    rows.clear();
    *t_d2h = std::chrono::steady_clock::now();
    HIP_TRY(hipMemsetAsync(M.head, 0, sizeof(MiHead), st));
    hipLaunchKernelGGL(ki_good, dim3(blocks(M.n_entries)), dim3(256), 0, st, M);
    for (size_t t = 0; t < tables.size(); ++t) {
        const MsTable &T = tables[t];
        const int n = T.k - 1;
        const uint8_t *in = M.good + T.off;
        uint32_t lo = 1;
        for (int s = 0; s < n; ++s) {
            const uint32_t hi = 1u << (2 * (n - 1 - s)), n_pass = hi * 15u * lo;
            uint8_t *to = s == n - 1 ? M.lattice + T.lat : mi.tmp[s & 1];
            hipLaunchKernelGGL(ki_widen, dim3(blocks(((int64_t)n_pass + 3) / 4)), dim3(256), 0, st, in, to, lo, n_pass);
            in = to;
            lo *= 15u;
        }
        hipLaunchKernelGGL(ki_maximal<false>, dim3(blocks(lo)), dim3(256), 0, st, M, (int)t, lo);
    }
    HIP_TRY(hipGetLastError());
    MiHead h = {};
    if (int rc = fetch_head(st, M.head, h)) return rc;
    if (!again) { I.n_good = (int64_t)h.n_good; I.n_pure = (int64_t)h.n_pure; I.n_maximal = (int64_t)h.n_maximal; }
    const int64_t NP = (int64_t)h.n_maximal;
    if (NP == 0) return 0;
    if (NP > mi.cap_pats) {
        if (!ms_fits((size_t)NP * (2 * sizeof(MiPat) + 16) + ((size_t)1 << 20))) return ms_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        if (pool.get(&M.pats, (size_t)NP) || pool.get(&M.rows, (size_t)NP) || pool.get(&M.flag, (size_t)NP * 2)) return -10;
        mi.cap_pats = NP;
    }
    M.place = M.flag + NP;
    M.n_pats = NP;
    for (size_t t = 0; t < tables.size(); ++t) {
        const uint32_t n_table = mi_pow15(tables[t].k - 1);
        hipLaunchKernelGGL(ki_maximal<true>, dim3(blocks(n_table)), dim3(256), 0, st, M, (int)t, n_table);
    }
    hipLaunchKernelGGL(ki_sums, dim3((unsigned)((NP + 3) / 4)), dim3(256), 0, st, M);
    hipLaunchKernelGGL(ki_pick, dim3(blocks(NP)), dim3(256), 0, st, M);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)M.flag, NP, M.place, &M.head->n_rows);
    hipLaunchKernelGGL(ki_gather, dim3(blocks(NP)), dim3(256), 0, st, M);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, M.head, h)) return rc;
    const int64_t NR = h.n_rows;
    if (!again) { S.n_selected = (int64_t)h.n_selected; S.n_rows = NR; }
    if (NR == 0) return 0;
    *t_d2h = std::chrono::steady_clock::now();
    rows.resize((size_t)NR);
    HIP_TRY(hipMemcpyAsync(rows.data(), M.rows, (size_t)NR * sizeof(MiPat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the order of the definition: tables stand in shape and j order, a table's indices in the order of the masks left to right
    std::sort(rows.begin(), rows.end(), [](const MiPat &a, const MiPat &b) {
        if (a.nM != b.nM) return a.nM > b.nM;
        const double fa = (double)a.nM / (double)a.nC, fb = (double)b.nM / (double)b.nC;
        if (fa != fb) return fa > fb;
        if (a.table != b.table) return a.table < b.table;
        return a.index < b.index;
    });
    return 0;
}

// a row's line -> false: mc_rowtext.h does not print the fraction
bool mi_line(MsText &text, const mc_motif_params &P, const std::vector<MsTable> &tables, const MiPat &r) {
    const MsTable &T = tables[(size_t)r.table];
    const char *shape = P.shapes[T.shape];
    uint32_t place = mi_pow15(T.k - 2);                                // of the first free X's digit
    for (int i = 0, x = 0; i < T.W; ++i) {
        if (shape[i] != 'X') { text.put('N'); continue; }
        if (x == T.j) text.put((char)P.base);
        else { text.put(" ACMGRSVTWYHKDBN"[r.index / place % 15u + 1]); place /= 15u; }
        ++x;
    }
    return ms_put_numbers(text, T.o, r.nG, r.nC, r.nM);
}
