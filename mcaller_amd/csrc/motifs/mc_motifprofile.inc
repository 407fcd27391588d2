// mc_motifprofile.inc -- motif methylation per bin (a contig, or a window of one) and every bin's nearest bins (part of
// mc_motifscan.hip; the definition: mcaller_amd/motif_profile.py; C ABI: mc_motif_profile, mc_motif_profile_last_stats,
// mc_motif_profile_release; Python: Device.motif_profile, motif_profile.motif_profile_device).
//
// The genome, the contig table and the two texts go through the motif finder's own kernels as they are: km_pack (the bit-planes,
// contigs 64-aligned with at least 32 bases of padding whose `valid` is 0: no occurrence of a motif of up to 32 letters spans two
// contigs), km_contigs, kp_count / kp_scan / kp_starts, km_parse (the methylated and control planes, the declines) and km_figures.
// Behind them:
//   kq_count     a lane per 64-bit word of the genome.  The A, C, G and T planes of the 128 bases around the word (32 before, 32
//                behind) from code0, code1 and valid; per motif and strand iu_window_marks (mc_iupac.h: the rule, for host and
//                device alike) -- exact for the word's 64 bases -- gives the sites; the marks are never written to memory.  The
//                popcounts of marks, marks & (meth | ctl) (the marks themselves without a control) and marks & meth, split where a
//                window's edge falls into the word (W >= 64: a word meets at most two bins of its contig), are added into 32-bit
//                counters [bin][motif][3] with integer atomics.  Where every word of a wave lies in one bin the three counts, 21
//                bits each in one 64-bit word (a wave's sum is below 2^14), are reduced across the wave first and lanes 0 to 2 issue
//                one atomic each per non-zero sum
//   kq_profile   a wave per bin, a lane per motif: the fraction, the defined flag (a ballot makes the bin's 64-bit mask), the
//                length of the row (mc_rowtext.h: RtCount)
//   kp_scan      the rows' offsets
//   kq_rows      a lane per (bin, motif): the row (RtStore) -- integers and the shortest round-trip double from mc_rowtext.h
//   kq_nn        THE HOT PATH, quadratic in the bins: a lane per query bin, a workgroup of one wave.  The query's fractions stand
//                in LDS ([motif][lane]: a lane's column, no bank conflict); the candidates are staged through LDS 16 at a time
//                (their fractions and masks, read by every lane at once: a broadcast) and walked in ascending index order; the
//                distance is the definition's -- over the set bits of (query mask & candidate mask) from the lowest: an fp64
//                subtraction, fabs and addition, the sum from 0.0, one division (the unit is compiled with contraction off).  The
//                lane's K best are kept sorted in LDS ([k][lane]) by an insertion under strict `<`: a later candidate never goes
//                before an equal earlier one, which is the index tie rule.  No atomic but the integer count of the pairs
//   kq_nn_sizes / kp_scan / kq_nn_rows   the second file the same way, a lane per (bin, place)
// No floating-point atomic anywhere; no atomic decides an order or a printed value.

constexpr int MQ_TILE = 16;                  // candidates of kq_nn in LDS at a time

struct MqHead {
    unsigned long long n_rows, n_defined, n_pairs, n_nn_rows;
    long long n_out_bytes, n_nn_bytes;
    int unprintable, pad;
};

struct MqArgs {
    const uint64_t *code0, *code1, *valid;
    const unsigned long long *meth[2], *ctl[2];
    int64_t n_words;
    const int64_t *gstart, *contig_len, *bin_first;      // bin_first: n_contigs + 1 entries
    int32_t n_contigs, n_motifs, has_control, K, min_shared, pad;
    int64_t window, min_sites, n_bins;
    const mc_iupac_motif *fwd, *rev;
    unsigned int *counts;                    // [bin][motif][3]
    double *frac;                            // [bin][motif], 0.0 where the motif is not defined
    unsigned long long *defined;             // [bin]
    const char *ids, *specs;
    const int64_t *id_off, *spec_off;
    long long *row_len, *row_off;            // [bin][motif]
    char *out;
    int32_t *nn_n, *nn_idx, *nn_shared;      // [bin], [bin][K]
    double *nn_d;
    long long *nn_len, *nn_off;              // [bin][K]
    char *nn_out;
    MqHead *head;
};

__device__ __forceinline__ iu_u128 mq_window(const uint64_t *plane, int64_t w) {
    const uint64_t before = plane[w - 1], mid = plane[w], behind = plane[w + 1];
    return (iu_u128)((before >> 32) | (mid << 32)) | ((iu_u128)((mid >> 32) | (behind << 32)) << 64);
}

__global__ __launch_bounds__(256) void kq_count(MqArgs P) {
    const int64_t w = 1 + (int64_t)blockIdx.x * 256 + threadIdx.x;      // (word 0 is padding; two words stand behind the genome)
    const int lane = threadIdx.x & 63;
    int64_t bin = -1, bin2 = -1;
    uint64_t first_mask = ~0ull;                                         // the word's bases that lie in `bin`; the others in bin2
    if (w < P.n_words - 2 && P.n_contigs > 0) {
        const int64_t g = w * 64;
        int lo = 0, hi = P.n_contigs;                                    // the last contig that begins at or before g
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (P.gstart[mid] <= g) lo = mid; else hi = mid;
        }
        const int64_t p = g - P.gstart[lo], L = P.contig_len[lo];
        if (p >= 0 && p < L) {
            if (P.window == 0) bin = lo;
            else {
                const int64_t i = p / P.window, edge = (i + 1) * P.window;
                bin = P.bin_first[lo] + i;
                if (edge < p + 64 && edge < L) { bin2 = bin + 1; first_mask = (1ull << (edge - p)) - 1ull; }
            }
        }
    }
    const uint64_t live = __ballot(bin >= 0);
    if (!live) return;                                                   // (the whole wave)
    const int64_t bin_a = __shfl(bin, __ffsll((unsigned long long)live) - 1);
    const bool one_bin = __ballot(bin >= 0 && (bin != bin_a || bin2 >= 0)) == 0;
    iu_u128 a = 0, c = 0, gg = 0, t = 0;
    uint64_t me[2] = {0, 0}, co[2] = {0, 0};
    if (bin >= 0) {
        const iu_u128 c0 = mq_window(P.code0, w), c1 = mq_window(P.code1, w), v = mq_window(P.valid, w);
        a = v & ~c0 & ~c1; c = v & c0 & ~c1; gg = v & ~c0 & c1; t = v & c0 & c1;
        for (int s = 0; s < 2; ++s) {
            me[s] = P.meth[s][w];
            co[s] = P.has_control ? (me[s] | P.ctl[s][w]) : ~0ull;
        }
    }
    for (int m = 0; m < P.n_motifs; ++m) {
        uint64_t pk = 0, pk2 = 0;                                        // nGenome | nCovered << 21 | nMethylated << 42
        if (bin >= 0) {
            const uint64_t mark[2] = {(uint64_t)(iu_window_marks(&P.fwd[m], a, c, gg, t) >> 32), (uint64_t)(iu_window_marks(&P.rev[m], a, c, gg, t) >> 32)};
            for (int s = 0; s < 2; ++s) {
                const uint64_t in1 = mark[s] & first_mask, in2 = mark[s] & ~first_mask;
                pk += (uint64_t)__popcll(in1) | ((uint64_t)__popcll(in1 & co[s]) << 21) | ((uint64_t)__popcll(in1 & me[s]) << 42);
                pk2 += (uint64_t)__popcll(in2) | ((uint64_t)__popcll(in2 & co[s]) << 21) | ((uint64_t)__popcll(in2 & me[s]) << 42);
            }
        }
        if (one_bin) {
            unsigned long long sum = pk;
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            const unsigned int part = (unsigned int)((sum >> (21 * lane)) & 0x1fffffull);
            if (lane < 3 && part) atomicAdd(&P.counts[((size_t)bin_a * P.n_motifs + m) * 3 + lane], part);
        } else if (bin >= 0) {
            for (int k = 0; k < 3; ++k) {
                const unsigned int p1 = (unsigned int)((pk >> (21 * k)) & 0x1fffffull), p2 = (unsigned int)((pk2 >> (21 * k)) & 0x1fffffull);
                if (p1) atomicAdd(&P.counts[((size_t)bin * P.n_motifs + m) * 3 + k], p1);
                if (p2) atomicAdd(&P.counts[((size_t)bin2 * P.n_motifs + m) * 3 + k], p2);
            }
        }
    }
}

// the bin's contig, start and end
__device__ __forceinline__ void mq_bin(const MqArgs &P, int64_t bin, int *contig, int64_t *start, int64_t *end) {
    if (P.window == 0) { *contig = (int)bin; *start = 0; *end = P.contig_len[bin]; return; }
    int lo = 0, hi = P.n_contigs;                                        // the last contig whose first bin is at or before `bin`
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.bin_first[mid] <= bin) lo = mid; else hi = mid;
    }
    *contig = lo;
    *start = (bin - P.bin_first[lo]) * P.window;
    *end = min(*start + P.window, P.contig_len[lo]);
}

template <class Sink>
__device__ __forceinline__ void mq_put_bin(Sink &o, const MqArgs &P, int64_t bin) {
    int contig;
    int64_t start, end;
    mq_bin(P, bin, &contig, &start, &end);
    for (int64_t i = P.id_off[contig]; i < P.id_off[contig + 1]; ++i) o.put(P.ids[i]);
    o.put('\t');
    rt_put_uint(o, (uint32_t)start); o.put('\t');
    rt_put_uint(o, (uint32_t)end); o.put('\t');
}

// a line of the profile file -> false: mc_rowtext.h does not print the fraction
template <class Sink>
__device__ __forceinline__ bool mq_row(Sink &o, const MqArgs &P, int64_t bin, int m, unsigned int nG, unsigned int nC, unsigned int nM) {
    mq_put_bin(o, P, bin);
    for (int64_t i = P.spec_off[m]; i < P.spec_off[m + 1]; ++i) o.put(P.specs[i]);
    o.put('\t');
    rt_put_uint(o, nG); o.put('\t');
    rt_put_uint(o, nC); o.put('\t');
    rt_put_uint(o, nM); o.put('\t');
    if (nC == 0) { o.put('N'); o.put('A'); }
    else if (!rt_put_repr(o, (double)nM / (double)nC)) return false;
    o.put('\n');
    return true;
}

__global__ __launch_bounds__(256) void kq_profile(MqArgs P) {
    const int64_t bin = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int m = threadIdx.x & 63;
    bool def = false, row = false;
    if (bin < P.n_bins && m < P.n_motifs) {
        const size_t at = (size_t)bin * P.n_motifs + m;
        const unsigned int nG = P.counts[at * 3], nC = P.has_control ? P.counts[at * 3 + 1] : nG, nM = P.counts[at * 3 + 2];
        def = nC > 0 && (long long)nC >= P.min_sites;
        P.frac[at] = def ? (double)nM / (double)nC : 0.0;
        long long len = 0;
        if (nG > 0) {
            RtCount n;
            if (!mq_row(n, P, bin, m, nG, nC, nM)) P.head->unprintable = 1;
            len = n.n;
            row = true;
        }
        P.row_len[at] = len;
    }
    const uint64_t mask = __ballot(def), rows = __ballot(row);
    if (m == 0 && bin < P.n_bins) {
        P.defined[bin] = mask;
        if (mask) atomicAdd(&P.head->n_defined, 1ull);
        if (rows) atomicAdd(&P.head->n_rows, (unsigned long long)__popcll(rows));
    }
}

__global__ __launch_bounds__(256) void kq_rows(MqArgs P) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= P.n_bins * P.n_motifs || P.row_len[at] == 0) return;
    const int64_t bin = at / P.n_motifs;
    const int m = (int)(at % P.n_motifs);
    const unsigned int nG = P.counts[at * 3], nC = P.has_control ? P.counts[at * 3 + 1] : nG, nM = P.counts[at * 3 + 2];
    RtStore o{P.out + P.row_off[at]};
    mq_row(o, P, bin, m, nG, nC, nM);
}

// dynamic LDS of kq_nn: the queries' fractions, a tile of candidates, the K best of every lane
inline size_t mq_nn_lds(int M, int K) { return ((size_t)M * 64 + (size_t)MQ_TILE * M + (size_t)K * 64) * 8 + (size_t)MQ_TILE * 8 + (size_t)K * 64 * 8; }

__global__ __launch_bounds__(64) void kq_nn(MqArgs P) {
    extern __shared__ double s_mq[];
    const int M = P.n_motifs, K = P.K, lane = threadIdx.x;
    double *s_q = s_mq;                                                  // [M][64]
    double *s_c = s_q + (size_t)M * 64;                                  // [MQ_TILE][M]
    double *s_d = s_c + (size_t)MQ_TILE * M;                             // [K][64]
    unsigned long long *s_cm = (unsigned long long *)(s_d + (size_t)K * 64);      // [MQ_TILE]
    int32_t *s_i = (int32_t *)(s_cm + MQ_TILE);                          // [K][64]
    int32_t *s_s = s_i + (size_t)K * 64;                                 // [K][64]
    const int64_t q = (int64_t)blockIdx.x * 64 + lane;
    const unsigned long long qmask = q < P.n_bins ? P.defined[q] : 0ull;
    for (int m = 0; m < M; ++m) s_q[m * 64 + lane] = q < P.n_bins ? P.frac[q * M + m] : 0.0;
    int n = 0;
    unsigned long long pairs = 0;
    for (int64_t c0 = 0; c0 < P.n_bins; c0 += MQ_TILE) {
        const int nt = (int)min((int64_t)MQ_TILE, P.n_bins - c0);
        __syncthreads();                                                 // (every lane is done with the tile before)
        for (int i = lane; i < nt * M; i += 64) s_c[i] = P.frac[c0 * M + i];
        if (lane < nt) s_cm[lane] = P.defined[c0 + lane];
        __syncthreads();
        if (!qmask) continue;
        for (int t = 0; t < nt; ++t) {
            const int64_t cand = c0 + t;
            unsigned long long S = qmask & s_cm[t];
            const int ns = __popcll(S);
            if (ns < P.min_shared || cand == q) continue;
            double sum = 0.0;
            while (S) {                                                  // ascending motif order
                const int m = __ffsll(S) - 1;
                S &= S - 1;
                sum += fabs(s_q[m * 64 + lane] - s_c[t * M + m]);
            }
            const double d = sum / (double)ns;
            ++pairs;
            if (n < K || d < s_d[(n - 1) * 64 + lane]) {
                int p = n < K ? n : K - 1;
                while (p > 0 && d < s_d[(p - 1) * 64 + lane]) {
                    s_d[p * 64 + lane] = s_d[(p - 1) * 64 + lane];
                    s_i[p * 64 + lane] = s_i[(p - 1) * 64 + lane];
                    s_s[p * 64 + lane] = s_s[(p - 1) * 64 + lane];
                    --p;
                }
                s_d[p * 64 + lane] = d; s_i[p * 64 + lane] = (int32_t)cand; s_s[p * 64 + lane] = ns;
                if (n < K) ++n;
            }
        }
    }
    if (q < P.n_bins) {
        P.nn_n[q] = n;
        for (int k = 0; k < n; ++k) {
            P.nn_d[q * K + k] = s_d[k * 64 + lane];
            P.nn_idx[q * K + k] = s_i[k * 64 + lane];
            P.nn_shared[q * K + k] = s_s[k * 64 + lane];
        }
    }
    unsigned long long lines = (unsigned long long)n;
    for (int o = 32; o > 0; o >>= 1) { pairs += __shfl_xor(pairs, o); lines += __shfl_xor(lines, o); }
    if (lane == 0) {
        if (pairs) atomicAdd(&P.head->n_pairs, pairs);
        if (lines) atomicAdd(&P.head->n_nn_rows, lines);
    }
}

// a line of the neighbours file -> false: mc_rowtext.h does not print the distance
template <class Sink>
__device__ __forceinline__ bool mq_nn_row(Sink &o, const MqArgs &P, int64_t bin, int64_t at) {
    mq_put_bin(o, P, bin);
    mq_put_bin(o, P, P.nn_idx[at]);
    rt_put_uint(o, (uint32_t)P.nn_shared[at]); o.put('\t');
    if (!rt_put_repr(o, P.nn_d[at])) return false;
    o.put('\n');
    return true;
}

__global__ __launch_bounds__(256) void kq_nn_sizes(MqArgs P) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= P.n_bins * P.K) return;
    const int64_t bin = at / P.K;
    long long len = 0;
    if ((int)(at % P.K) < P.nn_n[bin]) {
        RtCount n;
        if (!mq_nn_row(n, P, bin, at)) P.head->unprintable = 1;
        len = n.n;
    }
    P.nn_len[at] = len;
}

__global__ __launch_bounds__(256) void kq_nn_rows(MqArgs P) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= P.n_bins * P.K || P.nn_len[at] == 0) return;
    RtStore o{P.nn_out + P.nn_off[at]};
    mq_nn_row(o, P, at / P.K, at);
}

int mq_decline(mc_ctx *c, int32_t *status, int reason, int file, long long line) {
    static const char *const nouns[2] = {"bed", "control"};
    return decline_in_file(c->motif.profile_stats, status, "motif profile", ms_reason_text(reason), nouns, reason, file, line);
}

void mq_blank(mc_motif_profile_result *res) { *res = mc_motif_profile_result(); }

// Everything behind the uploads: A as ms_call fills it for the kernels of the motif finder that run here, P for the unit's own
int mq_run(mc_ctx *c, Pool &pool, MsArgs &A, MsHead *d_head, MqArgs &P, MqHead *d_mq, mc_motif_profile_result *res, int32_t *status) {
    mc_motif_profile_stats &S = c->motif.profile_stats;
    hipStream_t st = c->stream;
    const auto t_first = std::chrono::steady_clock::now();
    MsHead h = {};
    hipLaunchKernelGGL(km_pack, dim3((unsigned)(A.n_words * 64 / 256 + (A.n_words * 64 % 256 ? 1 : 0))), dim3(256), 0, st, A);
    if (A.n_contigs > 0) hipLaunchKernelGGL(km_contigs, dim3(blocks(A.n_contigs)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (A.n_bytes > 0) {
        long long *tile_off = nullptr, *line_start = nullptr;
        if (int rc = lines_count(pool, st, A.text, A.n_bytes, &d_head->kp, &tile_off)) return rc;
        if (int rc = fetch_head(st, d_head, h)) return rc;
        if (h.table_full) return mq_decline(c, status, MC_MOTIF_DECLINE_TABLE, 0, -1);
        A.n_nl = h.kp.n_newlines;
        if (too_many_lines(A.n_nl)) return mq_decline(c, status, MC_MOTIF_DECLINE_ROWS, 0, -1);
        if (!ms_fits(((size_t)A.n_nl + 2) * 8 + ((size_t)1 << 20))) return mq_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        if (int rc = lines_starts(pool, st, A.text, A.n_bytes, A.n_nl, tile_off, &d_head->kp, &line_start)) return rc;
        A.line_start = line_start;
        hipLaunchKernelGGL(km_parse, dim3(blocks(A.n_nl + 2)), dim3(256), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(km_figures, dim3(blocks(A.n_words)), dim3(256), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_head, h)) return rc;
    if (h.table_full) return mq_decline(c, status, MC_MOTIF_DECLINE_TABLE, 0, -1);
    if (A.n_bytes > 0) {
        S.n_lines1 = h.n_lines1; S.n_lines2 = h.kp.n_lines - h.n_lines1;
        if (h.decline != MS_NO_DECLINE) {
            const long long line = decline_line(h.decline);
            const bool first = line < h.n_lines1;
            return mq_decline(c, status, decline_reason(h.decline), first ? 1 : 2, first ? line : line - h.n_lines1);
        }
    }
    S.n_candidates = (int64_t)h.n_candidates; S.n_sites = (int64_t)h.n_sites; S.n_control = (int64_t)h.n_control;
    S.n_off_base = (int64_t)h.n_off_base;
    MqHead q = {};
    const int64_t B = P.n_bins, BM = B * P.n_motifs;
    if (B == 0) return 0;                                                // (no contig, or windows of contigs without bases: two empty files)
    // the counts, the fractions and the profile file
    if (A.n_words > 3) hipLaunchKernelGGL(kq_count, dim3(blocks(A.n_words - 3)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(kq_profile, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)P.row_len, BM, P.row_off, &d_mq->n_out_bytes);
    HIP_TRY(hipGetLastError());
    if (int rc = fetch_head(st, d_mq, q)) return rc;
    S.ms_counts = ms_since(t_first);
    if (q.unprintable) return mq_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
    S.n_rows = (int64_t)q.n_rows; S.n_defined = (int64_t)q.n_defined;
    if (!ms_fits((size_t)q.n_out_bytes + ((size_t)1 << 20))) return mq_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
    if (q.n_out_bytes > 0) {
        if (pool.get(&P.out, (size_t)q.n_out_bytes)) return -10;
        hipLaunchKernelGGL(kq_rows, dim3(blocks(BM)), dim3(256), 0, st, P);
        HIP_TRY(hipGetLastError());
    }
    // the neighbours
    long long n_nn_bytes = 0;
    if (P.K > 0) {
        const auto t_nn = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(kq_nn, dim3((unsigned)((B + 63) / 64)), dim3(64), mq_nn_lds(P.n_motifs, P.K), st, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        S.ms_neighbours = ms_since(t_nn);
        hipLaunchKernelGGL(kq_nn_sizes, dim3(blocks(B * P.K)), dim3(256), 0, st, P);
        hipLaunchKernelGGL(kp_scan, dim3(1), dim3(1024), 0, st, (const long long *)P.nn_len, B * P.K, P.nn_off, &d_mq->n_nn_bytes);
        HIP_TRY(hipGetLastError());
        if (int rc = fetch_head(st, d_mq, q)) return rc;
        if (q.unprintable) return mq_decline(c, status, MC_MOTIF_DECLINE_PRINT, 0, -1);
        S.n_pairs = (int64_t)q.n_pairs; S.n_nn_rows = (int64_t)q.n_nn_rows;
        n_nn_bytes = q.n_nn_bytes;
        if (!ms_fits((size_t)q.n_out_bytes + (size_t)n_nn_bytes + ((size_t)1 << 20))) return mq_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        if (n_nn_bytes > 0) {
            if (pool.get(&P.nn_out, (size_t)n_nn_bytes)) return -10;
            hipLaunchKernelGGL(kq_nn_rows, dim3(blocks(B * P.K)), dim3(256), 0, st, P);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    const auto t_d2h = std::chrono::steady_clock::now();
    if (int rc = fetch_out(c, c->motif.profile_out, P.out, (size_t)q.n_out_bytes, &res->out, &res->n_out)) return rc;
    if (int rc = fetch_out(c, c->motif.profile_nn, P.nn_out, (size_t)n_nn_bytes, &res->nn, &res->n_nn)) return rc;
    S.ms_d2h = ms_since(t_d2h);
    S.n_out_bytes = q.n_out_bytes; S.n_nn_bytes = n_nn_bytes;
    res->n_rows = S.n_rows; res->n_nn_rows = S.n_nn_rows;
    return 0;
}

bool mq_bad_params(const mc_motif_profile_params *Q) {
    if (!Q || Q->n_motifs < 1 || Q->n_motifs > MC_PROFILE_MAX_MOTIFS || !Q->letters || !Q->letters_off || !Q->called || !Q->specs || !Q->spec_off)
        return true;
    if (Q->window < 0 || (Q->window > 0 && Q->window < 64) || Q->min_sites < 1 || Q->min_shared < 1 || Q->neighbours < 0 ||
        Q->neighbours > MC_PROFILE_MAX_NEIGHBOURS || Q->letters_off[0] != 0 || Q->spec_off[0] != 0)
        return true;
    for (int i = 0; i < Q->n_motifs; ++i)
        if (Q->letters_off[i + 1] < Q->letters_off[i] || Q->spec_off[i + 1] < Q->spec_off[i]) return true;
    return false;
}

int mq_call(mc_ctx *c, const mc_ref_view *ref, const mc_text_source &s1, const mc_text_source *s2, const mc_motif_profile_params *Q,
            mc_motif_profile_result *res, int32_t *status) {
    mc_motif_profile_stats &S = c->motif.profile_stats;
    return pipeline_call(c, S, status, "motif profile", (size_t)32 << 20, [&] { mq_blank(res); }, [&](Call &K) -> int {
        Pool &pool = K.pool;
        S.n_bytes1 = s1.n_bytes; S.n_bytes2 = s2 ? s2->n_bytes : 0;
        const int M = Q->n_motifs, KN = Q->neighbours;
        const int base_code = Q->base == 'A' ? 0 : Q->base == 'C' ? 1 : Q->base == 'G' ? 2 : Q->base == 'T' ? 3 : -1;
        // the motifs of both strands by mc_iupac.h's own statement (iu_set_entry: the reverse complement, the mirrored offsets);
        // a called letter holds the base
        std::vector<mc_iupac_motif> motifs((size_t)2 * M);
        bool ok = base_code >= 0;
        for (int i = 0; i < M && ok; ++i) {
            mc_iupac_spec one = {};
            const int64_t lo = Q->letters_off[i], n = Q->letters_off[i + 1] - lo;
            ok = n >= 1 && n <= MC_IUPAC_MAX_LEN && iu_set_entry(&one, 0, Q->letters + lo, (int)n, Q->called[i]) == 0;
            for (int j = 0; j < n && ok; ++j)
                if ((Q->called[i] >> j) & 1u) ok = Q->letters[lo + j] == (char)Q->base;
            motifs[i] = one.fwd[0]; motifs[(size_t)M + i] = one.rev[0];
        }
        if (!ok) {
            mc_set_error("mc_motif_profile: a base other than A, C, G, T, or a motif that is none, calls no letter or calls a letter other than the base");
            return -12;
        }
        const int NC = ref->n_contigs;
        int64_t n_bases = 0;
        for (int i = 0; i < NC; ++i) n_bases += ref->contig_len[i];
        if (n_bases >= ((int64_t)1 << 31) || NC >= (1 << 24)) return mq_decline(c, status, MC_MOTIF_DECLINE_REFERENCE, 0, -1);
        // where the contigs stand (as in ms_call) and where their bins begin
        std::vector<int64_t> meta((size_t)NC * 4 + 2);
        int64_t G = 64, B = 0;
        for (int i = 0; i < NC; ++i) {
            const int64_t L = ref->contig_len[i];
            meta[i] = L; meta[NC + i] = ref->seq_off[i]; meta[2 * NC + i] = G; meta[3 * NC + i] = B;
            G = (G + L + 32 + 63) & ~(int64_t)63;
            B += Q->window == 0 ? 1 : (L + Q->window - 1) / Q->window;
        }
        meta[(size_t)4 * NC] = B;
        S.n_bins = B;
        const int64_t n_words = G / 64 + 2;
        const int64_t n_text = s1.n_bytes + (s2 ? s2->n_bytes : 0);
        const int64_t id_bytes = NC > 0 ? Q->contig_id_off[NC] : 0, spec_bytes = Q->spec_off[M];
        const uint64_t slots = table_slots(NC, 64, "MCALLER_MOTIF_TABLE_SLOTS");
        S.table_slots = (int64_t)slots;
        S.nn_lds_bytes = KN > 0 ? (int64_t)mq_nn_lds(M, KN) : 0;
        const size_t BM = (size_t)B * M, BK = (size_t)B * KN;
        const size_t need = (size_t)ref->n_seq_bytes + (size_t)n_words * 8 * 9 + (size_t)n_text + (size_t)id_bytes + (size_t)spec_bytes +
                            (size_t)NC * 48 + slots * 8 + BM * (12 + 8 + 16) + (size_t)B * 12 + BK * (8 + 8 + 16) + ((size_t)1 << 20);
        S.need_bytes = (int64_t)need;
        if (!ms_fits(need)) return mq_decline(c, status, MC_MOTIF_DECLINE_MEMORY, 0, -1);
        hipStream_t up = c->up_stream;
        MsArgs A = {};
        MqArgs P = {};
        uint8_t *d_seq = nullptr;
        int64_t *d_meta = nullptr, *d_id_off = nullptr, *d_spec_off = nullptr;
        char *d_ids = nullptr, *d_text = nullptr, *d_specs = nullptr;
        uint64_t *d_planes = nullptr;
        mc_iupac_motif *d_motifs = nullptr;
        MsHead *d_head = nullptr;
        MqHead *d_mq = nullptr;
        if (pool.get(&d_seq, (size_t)ref->n_seq_bytes + 1) || pool.get(&d_meta, meta.size()) || pool.get(&d_id_off, (size_t)NC + 1) ||
            pool.get(&d_ids, (size_t)id_bytes + 1) || pool.get(&d_text, (size_t)n_text + 1 + 64) || pool.get(&d_planes, (size_t)n_words * 9) ||
            pool.get(&d_motifs, motifs.size()) || pool.get(&d_specs, (size_t)spec_bytes + 1) || pool.get(&d_spec_off, (size_t)M + 1) ||
            pool.get(&d_head, 1) || pool.get(&d_mq, 1) || pool.get(&P.counts, BM * 3 + 1) || pool.get(&P.frac, BM + 1) ||
            pool.get(&P.defined, (size_t)B + 1) || pool.get(&P.row_len, BM + 1) || pool.get(&P.row_off, BM + 1))
            return -10;
        if (KN > 0 && (pool.get(&P.nn_n, (size_t)B + 1) || pool.get(&P.nn_idx, BK + 1) || pool.get(&P.nn_shared, BK + 1) || pool.get(&P.nn_d, BK + 1) ||
                       pool.get(&P.nn_len, BK + 1) || pool.get(&P.nn_off, BK + 1)))
            return -10;
        if (int rc = table_get(pool, up, &A.table, slots)) return rc;
        MsHead h = {};
        h.decline = MS_NO_DECLINE;
        const MqHead q = {};
        if (ref->n_seq_bytes > 0) HIP_TRY(hipMemcpyAsync(d_seq, ref->seq, (size_t)ref->n_seq_bytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, up));
        if (NC > 0) {
            HIP_TRY(hipMemcpyAsync(d_id_off, Q->contig_id_off, ((size_t)NC + 1) * 8, hipMemcpyHostToDevice, up));
            if (id_bytes > 0) HIP_TRY(hipMemcpyAsync(d_ids, Q->contig_ids, (size_t)id_bytes, hipMemcpyHostToDevice, up));
        }
        HIP_TRY(hipMemcpyAsync(d_motifs, motifs.data(), motifs.size() * sizeof(mc_iupac_motif), hipMemcpyHostToDevice, up));
        if (spec_bytes > 0) HIP_TRY(hipMemcpyAsync(d_specs, Q->specs, (size_t)spec_bytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_spec_off, Q->spec_off, ((size_t)M + 1) * 8, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_head, &h, sizeof h, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_mq, &q, sizeof q, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemsetAsync(d_planes + 5 * n_words, 0, (size_t)n_words * 4 * 8, up));             // methylated and control, both strands
        HIP_TRY(hipMemsetAsync(P.counts, 0, (BM * 3 + 1) * 4, up));
        HIP_TRY(hipStreamSynchronize(up));                                // (the host's vectors are the host's again)
        int64_t off2 = 0;
        if (int rc = K.feed.put_pair(s1, s2, d_text, &off2)) return rc;
        const int64_t n_bytes = s2 ? off2 + s2->n_bytes : s1.n_bytes;
        K.feed.times(S, K.t0);
        A.seq = d_seq; A.contig_len = d_meta; A.seq_off = d_meta + NC; A.gstart = d_meta + 2 * NC;
        A.n_contigs = NC; A.base_code = base_code; A.n_words = n_words;
        A.code0 = d_planes; A.code1 = d_planes + n_words; A.valid = d_planes + 2 * n_words;
        A.cand[0] = d_planes + 3 * n_words; A.cand[1] = d_planes + 4 * n_words;
        A.meth[0] = (unsigned long long *)(d_planes + 5 * n_words); A.meth[1] = (unsigned long long *)(d_planes + 6 * n_words);
        A.ctl[0] = (unsigned long long *)(d_planes + 7 * n_words); A.ctl[1] = (unsigned long long *)(d_planes + 8 * n_words);
        A.ids = d_ids; A.id_off = d_id_off; A.table_mask = slots - 1;
        const char *hm = getenv("MCALLER_MOTIF_HASH_MASK");
        A.hash_mask = hm && *hm ? strtoull(hm, nullptr, 16) : ~0ull;
        A.text = d_text; A.n_bytes = n_bytes; A.off2 = s2 ? off2 : n_bytes; A.head = d_head;
        A.has_control = s2 ? 1 : 0; A.G = G;
        P.code0 = A.code0; P.code1 = A.code1; P.valid = A.valid;
        for (int s = 0; s < 2; ++s) { P.meth[s] = A.meth[s]; P.ctl[s] = A.ctl[s]; }
        P.n_words = n_words; P.gstart = A.gstart; P.contig_len = A.contig_len; P.bin_first = d_meta + 3 * NC;
        P.n_contigs = NC; P.n_motifs = M; P.has_control = A.has_control; P.K = KN; P.min_shared = Q->min_shared;
        P.window = Q->window; P.min_sites = Q->min_sites; P.n_bins = B;
        P.fwd = d_motifs; P.rev = d_motifs + M;
        P.ids = d_ids; P.id_off = d_id_off; P.specs = d_specs; P.spec_off = d_spec_off;
        P.head = d_mq;
        const auto t_kernels = std::chrono::steady_clock::now();
        const int rc = mq_run(c, pool, A, d_head, P, d_mq, res, status);
        S.ms_kernels = ms_since(t_kernels) - S.ms_d2h;
        return rc;
    });
}
