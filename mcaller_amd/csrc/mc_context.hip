// mc_context.hip -- the life cycle of a context (create / destroy / sync, the NUMA binding of its process), the read qualities and
// the four classifier setters.  Host code only; the structures: mc_ctx.h.
#include "mc_ctx.h"

#include <memory>

// for the other translation units of the library (mc_train.hip)
int mc_internal_device(const mc_ctx *c) { return c->device; }
hipStream_t mc_internal_stream(const mc_ctx *c) { return c->stream; }
mc_forest_fit_stats *mc_internal_forest_stats(mc_ctx *c) { return &c->forest_stats; }

// Multi-GPU hosts: one process per GPU, and what a process copies out lands in ITS pinned memory.  Bound to the cores of the
// NUMA node the GPU hangs off, the process allocates there (first touch) and the DMA writes do not cross the socket link.
// -> the node (>= 0) when the calling thread was bound, -1 when the topology does not say (nothing changed).
extern "C" int mc_bind_to_device_numa_node(int device) {
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return -1;
    for (char *p = bus; *p; ++p) *p = (char)tolower((unsigned char)*p);
    char path[256];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    int node = -1;
    if (FILE *f = fopen(path, "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
    if (node < 0) return -1;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    char list[4096] = "";
    if (FILE *f = fopen(path, "r")) { if (!fgets(list, (int)sizeof(list), f)) list[0] = 0; fclose(f); }
    cpu_set_t *set = CPU_ALLOC(8192);
    if (!set) return -1;
    const size_t bytes = CPU_ALLOC_SIZE(8192);
    CPU_ZERO_S(bytes, set);
    int n_cpus = 0;
    for (char *p = list; *p;) {                       // "0-63,128-191"
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') { b = strtol(p + 1, &end, 10); p = end; }
        for (long cpu = a; cpu <= b && cpu < 8192; ++cpu) { CPU_SET_S((size_t)cpu, bytes, set); ++n_cpus; }
        while (*p == ',' || *p == '\n' || *p == ' ') ++p;
    }
    int rc = -1;
    if (n_cpus > 0 && sched_setaffinity(0, bytes, set) == 0) rc = node;
    CPU_FREE(set);
    return rc;
}

extern "C" int mc_ctx_create(int device, mc_ctx **out) {
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        mc_set_error("no HIP device available (%s): libmcaller_hip has no CPU fallback",
                     e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return -11;
    }
    if (device < 0 || device >= n) {
        mc_set_error("device %d out of range (%d visible)", device, n);
        return -11;
    }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<mc_ctx> c(new mc_ctx());                // (deleted, with what it holds by then, on every early return)
    c->device = device;
    for (Stream *s : {&c->stream, &c->copy_stream, &c->copy_stream2, &c->up_stream})
        if (int rc = s->create()) return rc;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        const int occ = mc_emit_occupancy();
        if (occ > 0) c->emit_wgs = occ;
        if (const char *e = getenv("MCALLER_EMIT_WGS")) { if (atoi(e) > 0) c->emit_wgs = atoi(e); }
        if (getenv("MCALLER_VERBOSE")) fprintf(stderr, "mcaller_hip: %d CUs, k1_emit occupancy %d workgroups/CU\n", c->n_cu, c->emit_wgs);
    }
    for (Event &ev : c->ev)
        if (int rc = ev.create()) return rc;
    if (c->own.get(&c->sync.cnt, 1)) return -10;
    HIP_TRY(hipMemset(c->sync.cnt, 0, sizeof(Counters)));
    *out = c.release();
    return 0;
}

// (the members of mc_ctx free what they hold, in the reverse of their order: mc_ctx.h)
extern "C" void mc_ctx_destroy(mc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)mc_sync_pass_streams(c);
    if (c->site_stream) (void)hipStreamSynchronize(c->site_stream);
    mc_comm_destroy(c);
    delete c;
}

extern "C" int mc_ctx_sync(mc_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    return mc_sync_pass_streams(c);
}

#define UP(dst, src, n, pool)                                                                          \
    do {                                                                                               \
        if (pool.get(&(dst), (size_t)(n)) != 0) return -10;                                            \
        if ((n) > 0) HIP_TRY(hipMemcpyAsync((void *)(dst), (src), (size_t)(n) * sizeof(*(dst)), hipMemcpyHostToDevice, c->stream)); \
    } while (0)

extern "C" int mc_ctx_set_read_quality(mc_ctx *c, const double *qual, int32_t n_reads) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = mc_sync_pass_streams(c)) return rc;            // passes in flight read the old buffer
    c->qual_allocs.clear();
    c->qual_own = nullptr;
    if (c->qual_allocs.get(&c->qual_own, (size_t)n_reads)) return -10;
    if (n_reads > 0) HIP_TRY(hipMemcpy(c->qual_own, qual, (size_t)n_reads * 8, hipMemcpyHostToDevice));
    c->qual = c->qual_own;
    c->n_qual = c->n_qual_own = n_reads;
    return 0;
}

extern "C" int mc_ctx_set_mlp(mc_ctx *c, int32_t n_models, int32_t n_in, int32_t n_hidden, const double *W1,
                              const double *b1, const double *W2, const double *b2, const uint8_t *sub_of_char) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = mc_sync_pass_streams(c)) return rc;            // (passes in flight score with the old one, on the side stream)
    if (n_in < 1 || n_in > MC_MAX_K + 1 || n_models < 1 || n_hidden < 1) {
        mc_set_error("unsupported MLP shape: %d models, %d inputs, %d hidden", n_models, n_in, n_hidden);
        return -12;
    }
    if (n_models > K2_MAXM) {
        mc_set_error("MLP with %d sub-models: k2_mlp lists at most %d", n_models, K2_MAXM);
        return -12;
    }
    c->clf.clear();
    DevMlp &M = c->clf.M;
    M.n_models = n_models;
    M.n_in = n_in;
    M.n_hidden = n_hidden;
    UP(M.W1, W1, (size_t)n_models * n_in * n_hidden, c->clf.pool);
    UP(M.b1, b1, (size_t)n_models * n_hidden, c->clf.pool);
    UP(M.W2, W2, (size_t)n_models * n_hidden, c->clf.pool);
    UP(M.b2, b2, (size_t)n_models, c->clf.pool);
    // unit by unit: the n_in weights into hidden unit j, its bias, its output weight (alive until the copy has been waited for)
    const size_t S = (size_t)n_in + 2;
    std::vector<double> wu((size_t)n_models * n_hidden * S);
    for (int m = 0; m < n_models; ++m)
        for (int j = 0; j < n_hidden; ++j) {
            double *u = &wu[((size_t)m * n_hidden + j) * S];
            for (int i = 0; i < n_in; ++i) u[i] = W1[((size_t)m * n_in + i) * n_hidden + j];
            u[n_in] = b1[(size_t)m * n_hidden + j];
            u[n_in + 1] = W2[(size_t)m * n_hidden + j];
        }
    UP(M.wu, wu.data(), wu.size(), c->clf.pool);
    // The fast forward (k2_mlp<.., true>): the same weights as floats, and per sub-model how far its probability can lie from
    // the fp64 one, as K0 + sum_i K_i |x_i|.  With u = 2^-24: a hidden unit's input a_j is off by at most g_dot sum_i |x_i W1_ij|
    // (+ the bias), g_dot = (n_in + 5) u (n_in products and sums, the inputs and weights rounded to float -- the weights after the factor
    // 2 log2(e) that makes the sum the exponent of tanh32s: a relative error either way); tanh is 1-Lipschitz and tanh32s is within
    // K2_TANH32_MAX_ERR of it; the output sum picks up g_acc sum_j |W2_j| (a quarter of the units per partial sum, two chains of
    // at most 13 terms and their sum, the products, the weights' rounding: g_acc = 29 u covers 25 in one chain); the logistic
    // function's slope is at most 1/4.  Five per cent on top for the float arithmetic the bound itself is evaluated in.
    const int h2 = (n_hidden + 1) / 2;
    std::vector<float> wp32((size_t)n_models * h2 * S * 2, 0.0f), margin((size_t)n_models * (MC_MAX_K + 2), 0.0f);    // (alive until the copies have been waited for)
    {
        const double c2 = 2.8853900817779268;         // 2 log2(e): the hidden unit's sum is the exponent of tanh32s
        for (int m = 0; m < n_models; ++m)
            for (int j = 0; j < n_hidden; ++j) {
                const double *uj = &wu[((size_t)m * n_hidden + j) * S];
                float *pj = &wp32[(((size_t)m * h2 + j / 2) * S) * 2 + (j & 1)];
                for (int i = 0; i <= n_in; ++i) pj[2 * i] = (float)(c2 * uj[i]);
                pj[2 * (n_in + 1)] = (float)uj[n_in + 1];
            }
        const double u = 5.9604644775390625e-08, g_dot = (n_in + 5.0) * u, g_acc = 29.0 * u;
        for (int m = 0; m < n_models; ++m) {
            double sw2 = 0.0, cb = 0.0, ci[MC_MAX_K + 1] = {0};
            for (int j = 0; j < n_hidden; ++j) {
                const double *uj = &wu[((size_t)m * n_hidden + j) * S];
                const double w2 = std::fabs(uj[n_in + 1]);
                sw2 += w2;
                cb += w2 * std::fabs(uj[n_in]);
                for (int i = 0; i < n_in; ++i) ci[i] += w2 * std::fabs(uj[i]);
            }
            float *mg = &margin[(size_t)m * (MC_MAX_K + 2)];
            mg[0] = (float)(1.05 * 0.25 * (sw2 * K2_TANH32_MAX_ERR + g_dot * cb + g_acc * sw2) + 1e-12);
            for (int i = 0; i < n_in; ++i) mg[1 + i] = (float)(1.05 * 0.25 * g_dot * ci[i]);
        }
        UP(M.wp32, wp32.data(), wp32.size(), c->clf.pool);
        UP(M.margin, margin.data(), margin.size(), c->clf.pool);
    }
    // (MCALLER_MLP_FP64=1: every record in fp64, as rounds 1-4 scored them)
    M.fast = (getenv("MCALLER_MLP_FP64") && atoi(getenv("MCALLER_MLP_FP64")) != 0) ? 0 : 1;
    UP(M.sub_of_char, sub_of_char, 256, c->clf.pool);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->clf.set(Classifier::MLP, n_in, M.sub_of_char);
    return 0;
}

extern "C" int mc_ctx_set_forest(mc_ctx *c, int32_t n_models, int32_t n_in, const int32_t *model_tree_off,
                                 const int32_t *tree_node_off, const int32_t *left, const int32_t *right,
                                 const int32_t *feature, const double *threshold, const double *value,
                                 const uint8_t *sub_of_char) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = mc_sync_pass_streams(c)) return rc;            // (passes in flight score with the old one, on the side stream)
    if (n_models < 1 || n_in < 1 || n_in > MC_MAX_K + 1) {
        mc_set_error("unsupported forest shape: %d models, %d inputs", n_models, n_in);
        return -12;
    }
    const int n_trees = model_tree_off[n_models];
    const int n_nodes = tree_node_off[n_trees];
    for (int i = 0; i < n_nodes; ++i)
        if (left[i] >= 0 && (feature[i] < 0 || feature[i] >= n_in || left[i] >= n_nodes || right[i] < 0 || right[i] >= n_nodes)) {
            mc_set_error("forest node %d is malformed", i);
            return -12;
        }
    c->clf.clear();
    DevForest &F = c->clf.F;
    F.n_models = n_models;
    F.n_in = n_in;
    UP(F.model_tree_off, model_tree_off, (size_t)n_models + 1, c->clf.pool);
    UP(F.tree_node_off, tree_node_off, (size_t)n_trees + 1, c->clf.pool);
    UP(F.left, left, (size_t)n_nodes, c->clf.pool);
    UP(F.right, right, (size_t)n_nodes, c->clf.pool);
    UP(F.feature, feature, (size_t)n_nodes, c->clf.pool);
    UP(F.threshold, threshold, (size_t)n_nodes, c->clf.pool);
    UP(F.value, value, (size_t)n_nodes * 2, c->clf.pool);
    UP(F.sub_of_char, sub_of_char, 256, c->clf.pool);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->clf.set(Classifier::FOREST, n_in, F.sub_of_char);
    return 0;
}

extern "C" int mc_ctx_set_simple_classifier(mc_ctx *c, int32_t kind, int32_t n_models, int32_t n_in, const double *params,
                                            int32_t stride, const uint8_t *sub_of_char) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = mc_sync_pass_streams(c)) return rc;            // (passes in flight score with the old one, on the side stream)
    const int want = kind == MC_CLF_LOGISTIC ? n_in + 1 : (kind == MC_CLF_GNB ? 4 * n_in + 2 : -1);
    if (n_models < 1 || n_in < 1 || n_in > MC_MAX_K + 1 || stride != want) {
        mc_set_error("unsupported classifier: kind %d, %d models, %d inputs, %d parameters each", kind, n_models, n_in, stride);
        return -12;
    }
    if (kind == MC_CLF_GNB)
        for (int m = 0; m < n_models; ++m)
            for (int cls = 0; cls < 2; ++cls)
                for (int i = 0; i < n_in; ++i)
                    if (!(params[(size_t)m * stride + (size_t)cls * 2 * n_in + n_in + i] > 0.0)) {
                        mc_set_error("naive Bayes model %d: variance %d of class %d is not positive", m, i, cls);
                        return -12;
                    }
    c->clf.clear();
    DevSimple &S = c->clf.Sc;
    UP(S.params, params, (size_t)n_models * stride, c->clf.pool);
    UP(S.sub_of_char, sub_of_char, 256, c->clf.pool);
    S.kind = kind; S.n_models = n_models; S.n_in = n_in; S.stride = stride;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->clf.set(Classifier::SIMPLE, n_in, S.sub_of_char);
    return 0;
}

extern "C" int mc_ctx_set_svm(mc_ctx *c, int32_t n_models, int32_t n_in, const int32_t *model_sv_off, const double *sv,
                              const double *dual_coef, const double *params, const uint8_t *sub_of_char) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = mc_sync_pass_streams(c)) return rc;            // (passes in flight score with the old one, on the side stream)
    if (n_models < 1 || n_models > K3S_MAXM || n_in < 1 || n_in > MC_MAX_K + 1 || model_sv_off[0] != 0) {
        mc_set_error("unsupported SVM shape: %d models (at most %d), %d inputs", n_models, K3S_MAXM, n_in);
        return -12;
    }
    for (int m = 0; m < n_models; ++m)
        if (model_sv_off[m + 1] <= model_sv_off[m] || !(params[4 * m] >= 0.0)) {
            mc_set_error("SVM sub-model %d: %d support vectors, gamma %g", m, model_sv_off[m + 1] - model_sv_off[m], params[4 * m]);
            return -12;
        }
    // the rows k3_svm stages: a support vector's coordinates, then its dual coefficient (alive until the copy has been waited for)
    const size_t n_sv = (size_t)model_sv_off[n_models], row = (size_t)n_in + 1;
    std::vector<double> rows(n_sv * row);
    for (size_t i = 0; i < n_sv; ++i) {
        memcpy(&rows[i * row], sv + i * n_in, (size_t)n_in * sizeof(double));
        rows[i * row + n_in] = dual_coef[i];
    }
    c->clf.clear();
    DevSvm &V = c->clf.Vs;
    UP(V.model_sv_off, model_sv_off, (size_t)n_models + 1, c->clf.pool);
    UP(V.sv, rows.data(), rows.size(), c->clf.pool);
    UP(V.params, params, (size_t)n_models * 4, c->clf.pool);
    UP(V.sub_of_char, sub_of_char, 256, c->clf.pool);
    V.n_models = n_models;
    V.n_in = n_in;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->clf.set(Classifier::SVM, n_in, V.sub_of_char);
    return 0;
}
