// mc_motifiter.inc -- find_motifs --iterative behind km_count (part of mc_motifscan.hip; the definition: mcaller_amd/find_motifs.py):
// print the first row, take the candidates it explains out of the candidate planes AND out of every table's counters, select again.
// Round 1 is the plain call; a later round costs the explained candidates x the tables, not the genome x the tables: planes, tables,
// lattices and their scratch stay on the device for the whole call, and no table is counted twice.
//   km_explain   a lane per base index, whole words per wave as in km_pack.  A lane whose base is a remaining candidate takes its
//                window's key from ms_key -- km_count's own validity test and letters: on '-' the mirrored offsets, both code bits
//                flipped -- and tests every free X's letter against that X's 4-bit set (8 sets in one 32-bit word; the called X
//                holds --base, or the lane were no candidate).  The wave ballots per strand; lane 0 clears the bits from cand[s][w] with a plain store
//                -- the wave owns the word, and no lane reads another word's candidates -- and the explained candidates go to a
//                list: one integer atomicAdd of the popcount per wave, each lane its own slot.  The order of the list shows nowhere
//   km_uncount   THE HOT PATH of rounds 2 on: a lane per (explained candidate, table), ONE launch for all tables, consecutive lanes
//                on consecutive tables of one candidate (they read the same plane words).  ms_key -- km_count's own test and key --
//                then 1 off nG, 1 off nM if the candidate is methylated, 1 off nC under km_count's condition: integer atomics in
//                global memory, so the tables equal a recount over the reduced candidate planes whatever the order of arrival
//   km_left      a lane per plane word: meth & cand of both strands, what no row explains, and its popcount
// The host checks the list's length against the row's nGenome (they are the same candidates: a mismatch is an internal error; n_list
// runs on through the rounds and a round's slots begin at its value before), has km_again zero the head's per-round counters and runs the selection of the mode again (ms_rows / mi_rows: in --iupac the good flags and the
// lattices are recomputed from the counters every round).

// n_before: the head's n_list when the launch begins (the counter runs through the rounds of a call; a round's list begins at 0)
__global__ __launch_bounds__(256) void km_explain(MsArgs A, int ti, uint32_t sets, unsigned long long n_before) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;       // (the grid covers whole words: n_words * 64 lanes)
    const int64_t w = g >> 6;
    const int bit = (int)(g & 63);
    const int lane = threadIdx.x & 63;
    const MsTable &T = A.tables[ti];
    bool hit = false;
    int s = 0;
    if (w < A.n_words) {
        const bool plus = (A.cand[0][w] >> bit) & 1ull, minus = (A.cand[1][w] >> bit) & 1ull;
        s = minus ? 1 : 0;
        uint32_t key;
        if ((plus || minus) && ms_key(A, T, g, s, &key)) {           // (a candidate stands inside a contig: g >= 64, two words behind)
            hit = true;
            for (int i = T.k - 1; i >= 0; --i) {                     // the key's lowest letter is the last free X's
                if (i == T.j) continue;                              // (the called letter is --base: the lane is a candidate)
                hit = hit && ((sets >> (4 * i + (key & 3u))) & 1u);
                key >>= 2;
            }
        }
    }
    const uint64_t bp = __ballot(hit && s == 0), bm = __ballot(hit && s == 1), both = bp | bm;
    if (!both) return;                                               // (the whole wave)
    unsigned long long first = 0;
    if (lane == 0) {
        if (bp) A.cand[0][w] &= ~bp;
        if (bm) A.cand[1][w] &= ~bm;
        first = atomicAdd(&A.head->n_list, (unsigned long long)__popcll(both));
    }
    first = __shfl(first, 0);
    if (hit) {
        const int64_t at = (int64_t)(first - n_before) + __popcll(both & ((1ull << lane) - 1ull));
        if (at < A.cap_list) A.list[at] = (long long)(g << 1 | s);   // (always: a base is on the list once in a call)
    }
}

// lanes [first, first + grid): lane = candidate * n_tables + table
__global__ __launch_bounds__(256) void km_uncount(MsArgs A, int64_t first, int64_t n_lanes) {
    const int64_t at = first + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n_lanes) return;
    const long long e = A.list[at / A.n_tables];
    const MsTable &T = A.tables[at % A.n_tables];
    const int64_t g = e >> 1, w = g >> 6;
    const int s = (int)(e & 1), bit = (int)(g & 63);
    uint32_t key;
    if (!ms_key(A, T, g, s, &key)) return;
    atomicSub(&A.nG[T.off + key], 1u);
    const bool is_meth = (A.meth[s][w] >> bit) & 1ull;
    if (is_meth) atomicSub(&A.nM[T.off + key], 1u);
    if (A.has_control && (is_meth || ((A.ctl[s][w] >> bit) & 1ull))) atomicSub(&A.nC[T.off + key], 1u);
}

__global__ __launch_bounds__(256) void km_left(MsArgs A) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long n = 0;
    if (w < A.n_words)
        for (int s = 0; s < 2; ++s) {
            const uint64_t left = A.meth[s][w] & A.cand[s][w];
            A.left[(int64_t)s * A.n_words + w] = left;
            n += __popcll(left);
        }
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&A.head->n_left, n);
}

// what --iterative needs on the device beside the mode's own: the list (a base is a candidate of one strand at most) and the two
// left-over planes
inline size_t it_need(int64_t n_bases, int64_t n_words, int64_t *list_bytes) {
    *list_bytes = n_bases * 8;
    return (size_t)n_bases * 8 + (size_t)n_words * 16;
}

// Everything behind km_count of an --iterative call.  A.list and A.left are allocated; t_first: when the first kernel was launched
int it_run(mc_ctx *c, Pool &pool, MsArgs &A, MsHead *d_head, const mc_motif_params &P, const std::vector<MsTable> &tables, bool iupac,
           int max_motifs, size_t scratch, std::chrono::steady_clock::time_point t_first, const char **out, int64_t *n_out, int64_t *n_rows,
           int32_t *status) {
    mc_motif_stats &S = c->motif.stats;
    mc_motif_iter_stats &I = c->motif.iter_stats;
    hipStream_t st = c->stream;
    MiState mi;
    if (iupac)
        if (int rc = mi_setup(pool, A, tables, scratch, mi)) return rc;
    MsText text;
    std::vector<MsRow> rows;
    std::vector<MiPat> pats;
    auto t_d2h = std::chrono::steady_clock::now();
    auto t_later = t_d2h;
    int rounds = 0;
    unsigned long long n_listed = 0;                                   // the head's n_list: every candidate explained so far
    for (;;) {
        // the report of this round; its first row as (table, the sets of its X, nGenome)
        int ti = 0;
        uint32_t sets = 0, nG = 0;
        if (iupac) {
            if (int rc = mi_rows(c, pool, mi, tables, rounds > 0, pats, &t_d2h, status)) return rc;
            if (*status != 0) return 0;
            if (pats.empty()) break;
            const MiPat &r = pats[0];
            if (!mi_line(text, P, tables, r)) return ms_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
            const MsTable &T = tables[(size_t)r.table];
            ti = r.table; nG = r.nG;
            uint32_t rest = r.index;
            for (int i = T.k - 1; i >= 0; --i) {                       // the last free X is the lowest digit
                if (i == T.j) { sets |= 1u << (4 * i + A.base_code); continue; }
                sets |= (rest % 15u + 1) << (4 * i);
                rest /= 15u;
            }
        } else {
            if (int rc = ms_rows(c, pool, A, d_head, rounds > 0, rows, &t_d2h, status)) return rc;
            if (*status != 0) return 0;
            if (rows.empty()) break;
            const MsRow &r = rows[0];
            if (!ms_line(text, P, tables, r)) return ms_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
            ti = (int)ms_table_of_entry(tables, r.entry); nG = r.nG;
            const MsTable &T = tables[(size_t)ti];
            uint32_t rest = r.entry - T.off;
            for (int i = T.k - 1; i >= 0; --i) {                       // the last free X is the key's lowest letter
                if (i == T.j) { sets |= 1u << (4 * i + A.base_code); continue; }
                sets |= 1u << (4 * i + (rest & 3u));
                rest >>= 2;
            }
        }
        I.n_explained[rounds++] = (int64_t)nG;
        if (rounds == 1) { I.ms_first_round = ms_since(t_first); t_later = std::chrono::steady_clock::now(); }
        // the explain step: out of the candidate planes (the last row's too: what is left is what no row explains) ...
        hipLaunchKernelGGL(km_explain, dim3((unsigned)(A.n_words * 64 / 256 + (A.n_words * 64 % 256 ? 1 : 0))), dim3(256), 0, st, A, ti, sets,
                           n_listed);
        HIP_TRY(hipGetLastError());
        MsHead h = {};
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.n_list - n_listed != (unsigned long long)nG || (int64_t)nG > A.cap_list) {
            // (what the planes say: km_figures adds the candidates that are left to the head's count of round 1)
            MsHead h2 = {};
            hipLaunchKernelGGL(km_figures, dim3(blocks(A.n_words)), dim3(256), 0, st, A);
            const int rc2 = fetch_head(st, d_head, h2);
            mc_set_error("motif finder: row %d of --iterative counts %u candidates and explains %llu (the planes hold %lld fewer than before the call)",
                         rounds, nG, h.n_list - n_listed, rc2 ? -1ll : (long long)(2 * h.n_candidates - h2.n_candidates));
            return -13;
        }
        n_listed = h.n_list;
        if (rounds == max_motifs) break;
        // ... and out of every table
        const int64_t n_lanes = (int64_t)nG * A.n_tables, step = (int64_t)1 << 30;
        for (int64_t first = 0; first < n_lanes; first += step)
            hipLaunchKernelGGL(km_uncount, dim3(blocks(std::min(step, n_lanes - first))), dim3(256), 0, st, A, first, n_lanes);
        HIP_TRY(hipGetLastError());
    }
    // what no row explains, into the context's pinned block
    hipLaunchKernelGGL(km_left, dim3(blocks(A.n_words)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    MsHead h = {};
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (rounds > 1) I.ms_later_rounds = ms_since(t_later);
    const size_t left_bytes = (size_t)A.n_words * 16;
    if (int rc = c->motif.left.need(left_bytes)) return rc;
    t_d2h = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(c->motif.left.get<uint64_t>(), A.left, left_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->motif.left_words = A.n_words;
    I.n_rounds = rounds;
    I.n_unexplained = (int64_t)h.n_left;
    S.n_rows = rounds;
    *n_rows = rounds;
    if (rounds == 0) return 0;
    return ms_hand_out(c, text, t_d2h, out, n_out);
}
