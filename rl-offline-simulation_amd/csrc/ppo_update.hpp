// The PPO update on the device (include/offsim.h: offsim_ppo_grad, offsim_ppo_update; PPOLearner.update): the loop of
// PPOAgentRevealed.adapt (offsim4rl/agents/ppo.py:162-223) -- Adam on the clipped surrogate with the KL early stop, then Adam on the value
// loss -- as pairs of launches, with no host round trip between them.
//
//   k_ppo_grad<KIND, XT>  one fused forward, loss and backward pass over M records.  A workgroup of 512 threads stages every layer's W^T
//                         and b into LDS once (pmlp_stage, policy_mlp.hpp) and then takes tiles of TM records (tile i of workgroup
//                         b is b + i * gridDim.x: a fixed assignment).  A tile's activations A [TM][all layers' widths] and back-propagated deltas D [TM][all layers'
//                         outputs] live in LDS and are never written to HBM.  Per tile:
//                           F  per layer, thread = (4 records, one output unit): one fmaf chain over k per record, W^T[k][j] read once
//                              for the four;
//                           O  thread = record: log-softmax, ratio, the clipped surrogate (or the squared error), the delta at the
//                              output, and the record's terms of n, loss, kl, entropy, clip count in f64 registers;
//                           B  per layer from the last, thread = (4 records, one input unit): D_prev = act'(h) * sum_j D[j] W^T[k][j];
//                           G  thread = up to 32 parameters (p = tid + 512 i, in registers for the whole launch):
//                              g[p] += sum_m D[m][j] * A[m][k], a bias's A column being a column of ones.
//                         Records with valid = 0 (and the tail of the last tile) get a zero delta at the output, so they add nothing.
//                         At the end the workgroup writes its partial gradient (f32 [P]) and its five partial sums (f64) to scratch.
//   k_ppo_adam<STEP>      one thread per parameter: the workgroups' partials summed in block order in f64 and divided by n (no float
//                         atomics: two runs give the same bits); STEP: torch.optim.Adam's default step in place.  Every block reduces
//                         the five sums the same way, so all of them take the same stop decision; block 0 records the pass.
//   k_ppo_finish          t += the steps taken.
// Early stop: an actor pass whose kl exceeds 1.5 * target_kl sets a flag in scratch instead of stepping; every later launch reads the
// flag first and returns.  Nothing waits on anything inside a kernel.
//
// A population (offsim_ppo_grad_pop, offsim_ppo_update_pop; POP instances of the same kernels) puts L independent learners on gridDim.y.
// Learner l = blockIdx.y has the stacked network l (pmlp_stage's lrn), the records m' = t * E + e of its E environments at memory index
// t * ld + l * E + e of the step-major [T, L * E] buffer (ppou_rec), its own scratch block (sized by the workgroups a learner really has,
// ppou_pop_stride) with its own stop flag and hyperparameters (k_ppo_pop_init writes them), and its own rows of m, v, t, stats and
// trace.  Tiles, their assignment to workgroups and every sum are those of the single learner on a contiguous [T * E] batch: same bits.
#pragma once

#define PPOU_THREADS 512
#define PPOU_OWN 32  // parameters per thread: OFFSIM_COLLECT_MLP_MAX_FLOATS / PPOU_THREADS
#define PPOU_RB 4    // records per thread in the F and B phases
static_assert(PPOU_OWN * PPOU_THREADS >= OFFSIM_COLLECT_MLP_MAX_FLOATS, "every parameter needs an owner");

struct PpoNet {
    float *W[PMLP_MAX_LAYERS];
    float *b[PMLP_MAX_LAYERS];
    int in[PMLP_MAX_LAYERS], out[PMLP_MAX_LAYERS];
    int goff[PMLP_MAX_LAYERS];  // flat parameter offset of the layer's W (its b follows)
    int woff[PMLP_MAX_LAYERS], boff[PMLP_MAX_LAYERS], ldw[PMLP_MAX_LAYERS];  // LDS: W^T [in][ldw] (ldw odd), b [out] (-1: none)
    int acol[PMLP_MAX_LAYERS + 1];  // A column of the layer's input (acol[n]: of the network's output)
    int dcol[PMLP_MAX_LAYERS];      // D column of the layer's output
    int n, P, act, lda, ldd, ones, w_floats;
    float slope;
};

struct PpoBatchArgs {
    const void *obs;
    const int32_t *act;
    const float *adv, *logp, *ret;
    const uint8_t *valid;
    int64_t M;
    int dO, TM;
    float clip_lo, clip_hi;
    int E;       // POP: environments per learner (M = T * E records per learner)
    int64_t ld;  // POP: the records' row stride, L * E
};

// scratch (doubles): [OFFSIM_PPO_MAX_BLOCKS][8] partial sums | 8 control | partial gradients f32 [OFFSIM_PPO_MAX_BLOCKS][P]
#define PPOU_CTRL (OFFSIM_PPO_MAX_BLOCKS * 8)
#define PPOU_GPART (PPOU_CTRL + 8)
// a population's scratch: per learner the same three parts for its nb workgroups, [nb][8] | 8 control | f32 [nb][P].  Control: the stop
// flag (u32), then lr, kl_limit (f64) and clip_lo, clip_hi (two f32 in one double's place).
__host__ __device__ __forceinline__ int64_t ppou_pop_stride(int nb, int P) { return OFFSIM_PPO_UPDATE_WORK_DOUBLES_NB(P, nb); }

// memory index of a learner's record m
template <bool POP>
__device__ __forceinline__ int64_t ppou_rec(const PpoBatchArgs &B, int64_t m, int lrn) {
    if constexpr (!POP) return m;
    else {
        const int64_t t = m / B.E;
        return t * B.ld + (int64_t)lrn * B.E + (m - t * B.E);
    }
}

__device__ __forceinline__ float ppou_dact(float h, int act, float slope) {  // the activation's derivative, from its output
    switch (act) {
        case OFFSIM_ACT_TANH: return 1.0f - h * h;
        case OFFSIM_ACT_RELU: return h > 0.0f ? 1.0f : 0.0f;
        case OFFSIM_ACT_LEAKY_RELU: return h > 0.0f ? 1.0f : slope;
        default: return 1.0f;
    }
}

template <int KIND, typename XT, bool POP = false>
__global__ void __launch_bounds__(PPOU_THREADS) k_ppo_grad(PpoNet N, PpoBatchArgs B, double *__restrict__ work) {
    const int lrn = POP ? (int)blockIdx.y : 0;
    const int ctrl = POP ? 8 * (int)gridDim.x : PPOU_CTRL;
    if constexpr (POP) work += (size_t)lrn * ppou_pop_stride((int)gridDim.x, N.P);
    if (*(volatile const uint32_t *)(work + ctrl) != 0u) return;  // the update stopped at an earlier pass
    float clip_lo = B.clip_lo, clip_hi = B.clip_hi;
    if constexpr (POP) {
        clip_lo = ((const float *)(work + ctrl + 3))[0];
        clip_hi = ((const float *)(work + ctrl + 3))[1];
    }
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float *w_lds = (float *)lds_raw;
    float *A = w_lds + N.w_floats;
    float *D = A + (size_t)B.TM * N.lda;
    double *red = (double *)(D + (((size_t)B.TM * N.ldd + 1) & ~(size_t)1));  // [TM][5] at the end
    const int tid = threadIdx.x, TM = B.TM, lda = N.lda, ldd = N.ldd, nl = N.n;
    const int nout = N.out[nl - 1];

    pmlp_stage(w_lds, N, N.ldw, tid, PPOU_THREADS, lrn);
    for (int e = tid; e < TM * lda; e += PPOU_THREADS) A[e] = 0.0f;
    for (int e = tid; e < TM * ldd; e += PPOU_THREADS) D[e] = 0.0f;
    __syncthreads();
    for (int m = tid; m < TM; m += PPOU_THREADS) A[m * lda + N.ones] = 1.0f;

    // the parameters this thread owns: p = tid + PPOU_THREADS * i -> (D column, A column) packed
    uint32_t own[PPOU_OWN];
    float g[PPOU_OWN];
    const int nown = (N.P + PPOU_THREADS - 1) / PPOU_THREADS;
#pragma unroll
    for (int i = 0; i < PPOU_OWN; i++) {
        g[i] = 0.0f;
        own[i] = 0xffffffffu;
        const int p = tid + PPOU_THREADS * i;
        if (p < N.P) {
            int l = 0;
            while (l + 1 < nl && p >= N.goff[l + 1]) l++;
            const int e = p - N.goff[l], nw = N.in[l] * N.out[l];
            int j, ac;
            if (e < nw) {
                j = e / N.in[l];
                ac = N.acol[l] + (e - j * N.in[l]);
            } else {
                j = e - nw;
                ac = N.ones;
            }
            own[i] = ((uint32_t)(N.dcol[l] + j) << 16) | (uint32_t)ac;
        }
    }
    double s_n = 0.0, s_loss = 0.0, s_kl = 0.0, s_ent = 0.0, s_clip = 0.0;  // of the records this thread is the O thread of

    const int64_t ntiles = (B.M + TM - 1) / TM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t m0 = tile * TM;
        const int tm = (int)(B.M - m0 < TM ? B.M - m0 : TM);
        // the tile's observations (0 past the end; an invalid record's row is zeros, whatever its obs holds)
        for (int e = tid; e < TM * B.dO; e += PPOU_THREADS) {
            const int m = e / B.dO, k = e - m * B.dO;
            const int64_t mi = m < tm ? ppou_rec<POP>(B, m0 + m, lrn) : 0;
            bool ok = m < tm && (!B.valid || B.valid[mi]);
            if constexpr (KIND == OFFSIM_PPO_ACTOR) {  // (an act outside [0, nA) makes the record invalid: its row is zeroed as well)
                if (ok) {
                    const int am = B.act[mi];
                    ok = am >= 0 && am < nout;
                }
            }
            A[m * lda + k] = ok ? pmlp_in<XT>((const XT *)B.obs, mi * B.dO + k) : 0.0f;
        }
        // the O thread's record
        bool ok = false;
        int a = 0;
        float adv = 0.0f, lpo = 0.0f, ret = 0.0f;
        if (tid < tm) {
            const int64_t mi = ppou_rec<POP>(B, m0 + tid, lrn);
            ok = !B.valid || B.valid[mi];
            if constexpr (KIND == OFFSIM_PPO_ACTOR) {
                a = B.act[mi];
                adv = B.adv[mi];
                lpo = B.logp[mi];
                if (a < 0 || a >= nout) ok = false;
            } else {
                ret = B.ret[mi];
            }
        }
        __syncthreads();
        // F
        for (int l = 0; l < nl; l++) {
            const int in = N.in[l], out = N.out[l], ldw = N.ldw[l];
            const float *wt = w_lds + N.woff[l];
            const float *x = A + N.acol[l];
            float *y = A + N.acol[l + 1];
            const bool last = l == nl - 1;
            for (int e = tid; e < (TM / PPOU_RB) * out; e += PPOU_THREADS) {
                const int mb = e / out, j = e - mb * out;
                const float *x0 = x + (size_t)(PPOU_RB * mb) * lda;
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                for (int k = 0; k < in; k++) {
                    const float w = wt[k * ldw + j];
                    c0 = fmaf(x0[k], w, c0);
                    c1 = fmaf(x0[lda + k], w, c1);
                    c2 = fmaf(x0[2 * lda + k], w, c2);
                    c3 = fmaf(x0[3 * lda + k], w, c3);
                }
                const float bj = N.boff[l] >= 0 ? w_lds[N.boff[l] + j] : 0.0f;
                float *y0 = y + (size_t)(PPOU_RB * mb) * lda + j;
                y0[0] = last ? c0 + bj : pmlp_act(c0 + bj, N.act, N.slope);
                y0[lda] = last ? c1 + bj : pmlp_act(c1 + bj, N.act, N.slope);
                y0[2 * lda] = last ? c2 + bj : pmlp_act(c2 + bj, N.act, N.slope);
                y0[3 * lda] = last ? c3 + bj : pmlp_act(c3 + bj, N.act, N.slope);
            }
            __syncthreads();
        }
        // O
        if (tid < TM) {
            const float *z = A + (size_t)tid * lda + N.acol[nl];
            float *d = D + (size_t)tid * ldd + N.dcol[nl - 1];
            if (!ok) {
                for (int j = 0; j < nout; j++) d[j] = 0.0f;
            } else if constexpr (KIND == OFFSIM_PPO_ACTOR) {
                float mx = z[0];
                for (int j = 1; j < nout; j++) mx = z[j] > mx ? z[j] : mx;
                float s = 0.0f;
                for (int j = 0; j < nout; j++) s = s + expf(z[j] - mx);
                const float lse = mx + logf(s);
                const float logp = z[a] - lse;
                const float ratio = expf(logp - lpo);
                const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
                const float x = ratio * adv, y = rc * adv;
                const bool inside = ratio >= clip_lo && ratio <= clip_hi;
                // d min(x, y) / d ratio: adv through x where x < y (or both, halved, where they are equal), through y inside the clip range
                const float gr = (inside || x < y) ? adv : 0.0f;
                const float dlogp = -gr * ratio;
                float ent = 0.0f;
                for (int j = 0; j < nout; j++) {
                    const float lj = z[j] - lse, pj = expf(lj);
                    ent = ent - pj * lj;
                    d[j] = dlogp * ((j == a ? 1.0f : 0.0f) - pj);
                }
                s_n += 1.0;
                s_loss += (double)(-fminf(x, y));
                s_kl += (double)(lpo - logp);
                s_ent += (double)ent;
                s_clip += inside ? 0.0 : 1.0;
            } else {
                const float e = z[0] - ret;
                d[0] = 2.0f * e;
                s_n += 1.0;
                s_loss += (double)(e * e);
            }
        }
        __syncthreads();
        // B
        for (int l = nl - 1; l >= 1; l--) {
            const int in = N.in[l], out = N.out[l], ldw = N.ldw[l];
            const float *wt = w_lds + N.woff[l];
            const float *dn = D + N.dcol[l];
            float *dp = D + N.dcol[l - 1];
            const float *h = A + N.acol[l];
            for (int e = tid; e < (TM / PPOU_RB) * in; e += PPOU_THREADS) {
                const int mb = e / in, k = e - mb * in;
                const float *d0 = dn + (size_t)(PPOU_RB * mb) * ldd;
                const float *wk = wt + k * ldw;
                float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
                for (int j = 0; j < out; j++) {
                    const float w = wk[j];
                    c0 = fmaf(d0[j], w, c0);
                    c1 = fmaf(d0[ldd + j], w, c1);
                    c2 = fmaf(d0[2 * ldd + j], w, c2);
                    c3 = fmaf(d0[3 * ldd + j], w, c3);
                }
                const float *h0 = h + (size_t)(PPOU_RB * mb) * lda + k;
                float *p0 = dp + (size_t)(PPOU_RB * mb) * ldd + k;
                p0[0] = c0 * ppou_dact(h0[0], N.act, N.slope);
                p0[ldd] = c1 * ppou_dact(h0[lda], N.act, N.slope);
                p0[2 * ldd] = c2 * ppou_dact(h0[2 * lda], N.act, N.slope);
                p0[3 * ldd] = c3 * ppou_dact(h0[3 * lda], N.act, N.slope);
            }
            __syncthreads();
        }
        // G
#pragma unroll
        for (int i = 0; i < PPOU_OWN; i++) {
            if (i < nown && own[i] != 0xffffffffu) {
                const float *dc = D + (own[i] >> 16), *ac = A + (own[i] & 0xffffu);
                float c = 0.0f;  // the tile's sum on its own, then one add: shorter chains than one running sum over every tile
                for (int m = 0; m < TM; m++) c = fmaf(dc[(size_t)m * ldd], ac[(size_t)m * lda], c);
                g[i] = g[i] + c;
            }
        }
        __syncthreads();
    }
    float *gpart = (float *)(work + ctrl + 8) + (size_t)blockIdx.x * N.P;
#pragma unroll
    for (int i = 0; i < PPOU_OWN; i++) {
        const int p = tid + PPOU_THREADS * i;
        if (p < N.P) gpart[p] = g[i];
    }
    if (tid < TM) {
        red[tid * 5 + 0] = s_n;
        red[tid * 5 + 1] = s_loss;
        red[tid * 5 + 2] = s_kl;
        red[tid * 5 + 3] = s_ent;
        red[tid * 5 + 4] = s_clip;
    }
    __syncthreads();
    if (tid < 5) {
        double s = 0.0;
        for (int m = 0; m < TM; m++) s += red[m * 5 + tid];
        work[(size_t)blockIdx.x * 8 + tid] = s;
    }
}

struct PpoAdamArgs {
    float *m, *v;
    const int64_t *t;
    double lr, kl_limit;
    double *stats, *trace;  // update: stats [6], trace [iters][2]; grad: stats [5]
    float *grad_out;
    int iter, kind, nblocks;
    int iters;  // POP: the rows of a learner's trace
};

#define PPOU_ADAM_BLOCK 256

template <bool STEP, bool POP = false>
__global__ void __launch_bounds__(PPOU_ADAM_BLOCK) k_ppo_adam(PpoNet N, PpoAdamArgs O, double *__restrict__ work) {
    const int lrn = POP ? (int)blockIdx.y : 0;
    const int ctrl = POP ? 8 * O.nblocks : PPOU_CTRL;
    if constexpr (POP) {  // the learner's scratch, hyperparameters and rows of the outputs and the optimiser state
        work += (size_t)lrn * ppou_pop_stride(O.nblocks, N.P);
        O.lr = work[ctrl + 1];
        O.kl_limit = work[ctrl + 2];
        O.stats += (size_t)lrn * (STEP ? 6 : 5);
        if (STEP) {
            O.trace += (size_t)lrn * O.iters * 2;
            O.m += (size_t)lrn * N.P;
            O.v += (size_t)lrn * N.P;
            O.t += lrn;
        } else {
            O.grad_out += (size_t)lrn * N.P;
        }
    }
    volatile uint32_t *stop_flag = (volatile uint32_t *)(work + ctrl);
    if (STEP && *stop_flag != 0u) return;
    __shared__ double sh[5];
    if (threadIdx.x < 5) {
        double s = 0.0;
        for (int b = 0; b < O.nblocks; b++) s += work[(size_t)b * 8 + threadIdx.x];
        sh[threadIdx.x] = s;
    }
    __syncthreads();
    const double n = sh[0];
    const double loss = n > 0.0 ? sh[1] / n : 0.0, kl = n > 0.0 ? sh[2] / n : 0.0, ent = n > 0.0 ? sh[3] / n : 0.0, cf = n > 0.0 ? sh[4] / n : 0.0;
    const bool stop = STEP && (n == 0.0 || (O.kind == OFFSIM_PPO_ACTOR && kl > O.kl_limit));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if constexpr (STEP) {
            O.trace[2 * O.iter + 0] = loss;
            O.trace[2 * O.iter + 1] = kl;
            if (O.iter == 0) {
                O.stats[0] = loss;
                O.stats[3] = ent;
            }
            O.stats[1] = loss;
            O.stats[2] = kl;
            O.stats[4] = cf;
            O.stats[5] = (double)O.iter;
            if (stop) *stop_flag = 1u;
        } else {
            O.stats[0] = n;
            O.stats[1] = loss;
            O.stats[2] = kl;
            O.stats[3] = ent;
            O.stats[4] = cf;
        }
    }
    if (stop) return;
    const int p = blockIdx.x * PPOU_ADAM_BLOCK + threadIdx.x;
    if (p >= N.P) return;
    const float *gpart = (const float *)(work + ctrl + 8);
    double gs = 0.0;
    for (int b = 0; b < O.nblocks; b++) gs += (double)gpart[(size_t)b * N.P + p];
    const double gd = n > 0.0 ? gs / n : 0.0;
    if constexpr (!STEP) {
        O.grad_out[p] = (float)gd;
    } else {
        int l = 0;
        while (l + 1 < N.n && p >= N.goff[l + 1]) l++;
        const int e = p - N.goff[l], nw = N.in[l] * N.out[l];
        float *q = e < nw ? N.W[l] + (size_t)lrn * nw + e : N.b[l] + (size_t)lrn * N.out[l] + (e - nw);
        // torch.optim.Adam, defaults: b1 = 0.9, b2 = 0.999, eps = 1e-8, no weight decay; f64 arithmetic on the f32 state
        const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
        const double t = (double)(*O.t + O.iter + 1);
        // m and v are rounded to the f32 state first and the step reads them back from it, as torch's does
        const float mf = (float)(b1 * (double)O.m[p] + (1.0 - b1) * gd);
        const float vf = (float)(b2 * (double)O.v[p] + (1.0 - b2) * gd * gd);
        const double step = O.lr / (1.0 - pow(b1, t));
        const double den = sqrt((double)vf) / sqrt(1.0 - pow(b2, t)) + eps;
        O.m[p] = mf;
        O.v[p] = vf;
        *q = (float)((double)*q - step * (double)mf / den);
    }
}

// after the last pair: t += the steps taken (StopIter steps if the update stopped, else iters)
__global__ void k_ppo_finish(int64_t *t, const double *stats, const double *work, int iters) {
    const bool stopped = *(const uint32_t *)(work + PPOU_CTRL) != 0u;
    *t += stopped ? (int64_t)stats[5] : (int64_t)iters;
}
// the same for every learner of a population (its flag at work + l * stride + ctrl)
__global__ void k_ppo_finish_pop(int64_t *t, const double *stats, const double *work, int iters, int L, int64_t stride, int ctrl) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const bool stopped = *(const uint32_t *)(work + (size_t)l * stride + ctrl) != 0u;
    t[l] += stopped ? (int64_t)stats[6 * (size_t)l + 5] : (int64_t)iters;
}

// A population's control blocks: the stop flags cleared and the learners' hyperparameters, PPOU_POP_CHUNK learners per launch by value
// (host arrays reach the device without a copy the host would have to wait for).
#define PPOU_POP_CHUNK 64
struct PpoPopHyper {
    double lr[PPOU_POP_CHUNK], kl_limit[PPOU_POP_CHUNK];
    float clip_lo[PPOU_POP_CHUNK], clip_hi[PPOU_POP_CHUNK];
    int l0, n;
};
__global__ void k_ppo_pop_init(PpoPopHyper H, double *work, int64_t stride, int ctrl) {
    const int i = threadIdx.x;
    if (i >= H.n) return;
    double *c = work + (size_t)(H.l0 + i) * stride + ctrl;
    *(uint64_t *)c = 0ull;
    c[1] = H.lr[i];
    c[2] = H.kl_limit[i];
    ((float *)(c + 3))[0] = H.clip_lo[i];
    ((float *)(c + 3))[1] = H.clip_hi[i];
}

// The network (pmlp_describe's checks) and the batch of an update, and k_ppo_grad's / k_ppo_adam's layouts of them.
static int ppou_prepare(const char *who, const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *bt, PpoNet &N, PpoBatchArgs &B, size_t &lds) {
    if (!net || !bt) return fail(OFFSIM_EINVAL, "%s: net / batch is NULL", who);
    if (kind != OFFSIM_PPO_ACTOR && kind != OFFSIM_PPO_CRITIC) return fail(OFFSIM_EINVAL, "%s: kind must be OFFSIM_PPO_ACTOR or OFFSIM_PPO_CRITIC", who);
    PmlpNet D;
    int rc = pmlp_describe(who, net->layers_host, net->n_layers, bt->dO, net->activation, net->slope, bt->x_dtype,
                           kind == OFFSIM_PPO_CRITIC ? 1 : PMLP_OUT_ACTIONS, D);
    if (rc) return rc;
    if (D.act == OFFSIM_ACT_LEAKY_RELU && !(D.slope >= 0.0f)) return fail(OFFSIM_EINVAL, "%s: a leaky_relu slope below 0 is not supported", who);
    if (bt->M < 0) return fail(OFFSIM_EINVAL, "%s: M must be >= 0", who);
    memset(&N, 0, sizeof(N));
    memset(&B, 0, sizeof(B));
    const int n = D.n;
    int P = 0, wf = 0, ac = D.dO, dc = 0;
    for (int l = 0; l < n; l++) {
        const offsim_ppo_layer &y = net->layers_host[l];  // (the writable pointers)
        N.W[l] = y.W;
        N.b[l] = y.b;
        N.in[l] = y.in;
        N.out[l] = y.out;
        N.goff[l] = P;
        P += y.in * y.out + (y.b ? y.out : 0);
        N.ldw[l] = y.out | 1;
        N.woff[l] = wf;
        wf += y.in * N.ldw[l];
        N.boff[l] = y.b ? wf : -1;
        wf += y.b ? y.out : 0;
        N.acol[l] = l == 0 ? 0 : ac;
        if (l > 0) ac += y.in;
        N.dcol[l] = dc;
        dc += y.out;
    }
    if (P > OFFSIM_COLLECT_MLP_MAX_FLOATS) return fail(OFFSIM_EUNSUPPORTED, "%s: the network's weights exceed OFFSIM_COLLECT_MLP_MAX_FLOATS", who);
    N.acol[n] = ac;
    ac += N.out[n - 1];
    N.ones = ac;
    N.lda = (ac + 1) | 1;
    N.ldd = dc | 1;
    N.n = n;
    N.P = P;
    N.act = D.act;
    N.slope = D.slope;
    N.w_floats = (wf + 3) & ~3;
    int TM = 32;
    for (;; TM /= 2) {
        lds = sizeof(float) * ((size_t)N.w_floats + (size_t)TM * N.lda + (((size_t)TM * N.ldd + 1) & ~(size_t)1)) + sizeof(double) * 5 * TM;
        if (lds <= 160 * 1024 || TM == PPOU_RB) break;
    }
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the weights and one tile's activations exceed 160 KiB of LDS", who);
    if (bt->M > 0) {
        if (!bt->obs) return fail(OFFSIM_EINVAL, "%s: obs is NULL", who);
        if (kind == OFFSIM_PPO_ACTOR && (!bt->act || !bt->adv || !bt->logp)) return fail(OFFSIM_EINVAL, "%s: the actor needs act, adv and logp", who);
        if (kind == OFFSIM_PPO_CRITIC && !bt->ret) return fail(OFFSIM_EINVAL, "%s: the critic needs ret", who);
    }
    B.obs = bt->obs;
    B.act = bt->act;
    B.adv = bt->adv;
    B.logp = bt->logp;
    B.ret = bt->ret;
    B.valid = bt->valid;
    B.M = bt->M;
    B.dO = D.dO;
    B.TM = TM;
    return OFFSIM_OK;
}

static unsigned ppou_blocks(const PpoBatchArgs &B) {
    const int64_t nt = B.M / B.TM + (B.M % B.TM != 0);  // (no overflow at any M: the sizing function takes INT64_MAX)
    return (unsigned)(nt < OFFSIM_PPO_MAX_BLOCKS ? nt : OFFSIM_PPO_MAX_BLOCKS);
}

// POP: L learners on gridDim.y (B.M, B.E, B.ld: a learner's records)
template <bool POP = false>
static int ppou_launch_grad(int32_t kind, int32_t x_dtype, const PpoNet &N, const PpoBatchArgs &B, size_t lds, double *work, hipStream_t s, int L = 1) {
    dim3 grid(ppou_blocks(B), (unsigned)L), block(PPOU_THREADS);
#define LAUNCH_PPOU(KIND, XT)                                                                     \
    do {                                                                                          \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_ppo_grad<KIND, XT, POP>), (int)lds));       \
        hipLaunchKernelGGL((k_ppo_grad<KIND, XT, POP>), grid, block, lds, s, N, B, work);         \
    } while (0)
    if (kind == OFFSIM_PPO_ACTOR) {
        if (x_dtype == OFFSIM_F32) LAUNCH_PPOU(OFFSIM_PPO_ACTOR, float);
        else LAUNCH_PPOU(OFFSIM_PPO_ACTOR, __half);
    } else {
        if (x_dtype == OFFSIM_F32) LAUNCH_PPOU(OFFSIM_PPO_CRITIC, float);
        else LAUNCH_PPOU(OFFSIM_PPO_CRITIC, __half);
    }
#undef LAUNCH_PPOU
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

static bool ppou_clip_ok(double c) { return c >= 0.0 && c < 1.0; }

extern "C" int64_t offsim_ppo_update_work_doubles(const offsim_ppo_net *net) {
    if (!net || !net->layers_host || net->n_layers < 1 || net->n_layers > PMLP_MAX_LAYERS)
        return fail(OFFSIM_EINVAL, "ppo_update_work_doubles: 1 to 4 Linear layers%s");
    int64_t P = 0;
    for (int l = 0; l < net->n_layers; l++) {
        const offsim_ppo_layer &y = net->layers_host[l];
        if (y.in < 1 || y.out < 1 || y.in > PMLP_MAX_HIDDEN || y.out > PMLP_MAX_HIDDEN) return fail(OFFSIM_EINVAL, "ppo_update_work_doubles: bad layer widths%s");
        P += (int64_t)y.in * y.out + (y.b ? y.out : 0);
    }
    return OFFSIM_PPO_UPDATE_WORK_DOUBLES(P);
}

extern "C" int offsim_ppo_grad(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, double clip_ratio, float *grad, double *stats,
                               double *work, void *stream) {
    PpoNet N;
    PpoBatchArgs B;
    size_t lds;
    int rc = ppou_prepare("ppo_grad", net, kind, batch, N, B, lds);
    if (rc) return rc;
    if (!ppou_clip_ok(clip_ratio)) return fail(OFFSIM_EINVAL, "ppo_grad: clip_ratio must be in [0, 1)%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!grad || !stats || !work) return fail(OFFSIM_EINVAL, "ppo_grad: grad / stats / work is NULL%s");
    B.clip_lo = (float)(1.0 - clip_ratio);
    B.clip_hi = (float)(1.0 + clip_ratio);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(work + PPOU_CTRL, 0, 8 * sizeof(double), s));
    rc = ppou_launch_grad(kind, batch->x_dtype, N, B, lds, work, s);
    if (rc) return rc;
    PpoAdamArgs O;
    memset(&O, 0, sizeof(O));
    O.stats = stats;
    O.grad_out = grad;
    O.kind = kind;
    O.nblocks = (int)ppou_blocks(B);
    hipLaunchKernelGGL((k_ppo_adam<false>), dim3((N.P + PPOU_ADAM_BLOCK - 1) / PPOU_ADAM_BLOCK), dim3(PPOU_ADAM_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_ppo_update(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, double clip_ratio, double target_kl,
                                 int32_t iters, const offsim_ppo_adam *opt, double *stats, double *trace, double *work, void *stream) {
    PpoNet N;
    PpoBatchArgs B;
    size_t lds;
    int rc = ppou_prepare("ppo_update", net, kind, batch, N, B, lds);
    if (rc) return rc;
    if (!ppou_clip_ok(clip_ratio)) return fail(OFFSIM_EINVAL, "ppo_update: clip_ratio must be in [0, 1)%s");
    if (!(target_kl >= 0.0)) return fail(OFFSIM_EINVAL, "ppo_update: target_kl must be >= 0%s");
    if (iters < 0) return fail(OFFSIM_EINVAL, "ppo_update: iters must be >= 0%s");
    if (!opt || !(opt->lr >= 0.0)) return fail(OFFSIM_EINVAL, "ppo_update: opt is NULL or its lr is negative%s");
    if (B.M == 0 || iters == 0) return OFFSIM_OK;
    if (!opt->m || !opt->v || !opt->t) return fail(OFFSIM_EINVAL, "ppo_update: opt->m / v / t is NULL%s");
    if (!stats || !trace || !work) return fail(OFFSIM_EINVAL, "ppo_update: stats / trace / work is NULL%s");
    B.clip_lo = (float)(1.0 - clip_ratio);
    B.clip_hi = (float)(1.0 + clip_ratio);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(work + PPOU_CTRL, 0, 8 * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(trace, 0xff, (size_t)iters * 2 * sizeof(double), s));  // passes that never ran stay NaN
    PpoAdamArgs O;
    memset(&O, 0, sizeof(O));
    O.m = opt->m;
    O.v = opt->v;
    O.t = opt->t;
    O.lr = opt->lr;
    O.kl_limit = 1.5 * target_kl;
    O.stats = stats;
    O.trace = trace;
    O.kind = kind;
    O.nblocks = (int)ppou_blocks(B);
    const dim3 agrid((N.P + PPOU_ADAM_BLOCK - 1) / PPOU_ADAM_BLOCK);
    for (int i = 0; i < iters; i++) {
        rc = ppou_launch_grad(kind, batch->x_dtype, N, B, lds, work, s);
        if (rc) return rc;
        O.iter = i;
        hipLaunchKernelGGL((k_ppo_adam<true>), agrid, dim3(PPOU_ADAM_BLOCK), 0, s, N, O, work);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(1), 0, s, opt->t, (const double *)stats, (const double *)work, (int)iters);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// ---- a population of L learners (include/offsim.h: offsim_ppo_grad_pop, offsim_ppo_update_pop) ----

// ppou_prepare for a population: batch->M = T * L * E records of the step-major [T, L * E] buffer; B describes ONE learner's T * E.
static int ppou_prepare_pop(const char *who, const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *bt, int32_t L, int32_t E, PpoNet &N,
                            PpoBatchArgs &B, size_t &lds) {
    if (L <= 0 || E <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535 and E >= 1", who);
    int rc = ppou_prepare(who, net, kind, bt, N, B, lds);
    if (rc) return rc;
    if (bt->M % ((int64_t)L * E) != 0) return fail(OFFSIM_EINVAL, "%s: M must be T * L * E", who);
    B.M = bt->M / L;
    B.E = E;
    B.ld = (int64_t)L * E;
    return OFFSIM_OK;
}

// the control blocks of all learners; lr / target_kl NULL (offsim_ppo_grad_pop): zeros
static int ppou_pop_init(int L, const double *lr, const double *clip_ratio, const double *target_kl, double *work, int64_t stride, int ctrl, hipStream_t s) {
    for (int l0 = 0; l0 < L; l0 += PPOU_POP_CHUNK) {
        PpoPopHyper H;
        memset(&H, 0, sizeof(H));
        H.l0 = l0;
        H.n = L - l0 < PPOU_POP_CHUNK ? L - l0 : PPOU_POP_CHUNK;
        for (int i = 0; i < H.n; i++) {
            H.lr[i] = lr ? lr[l0 + i] : 0.0;
            H.kl_limit[i] = target_kl ? 1.5 * target_kl[l0 + i] : 0.0;
            H.clip_lo[i] = (float)(1.0 - clip_ratio[l0 + i]);
            H.clip_hi[i] = (float)(1.0 + clip_ratio[l0 + i]);
        }
        hipLaunchKernelGGL(k_ppo_pop_init, dim3(1), dim3(PPOU_POP_CHUNK), 0, s, H, work, stride, ctrl);
        LAUNCH_CHECK();
    }
    return OFFSIM_OK;
}

extern "C" int64_t offsim_ppo_update_work_doubles_pop(const offsim_ppo_net *net, int32_t L, int64_t M) {
    if (!net || !net->layers_host || net->n_layers < 1) return fail(OFFSIM_EINVAL, "ppo_update_work_doubles_pop: net is NULL or has no layers%s");
    if (L <= 0 || M < 0) return fail(OFFSIM_EINVAL, "ppo_update_work_doubles_pop: L must be >= 1 and M >= 0%s");
    offsim_ppo_batch bt;
    memset(&bt, 0, sizeof(bt));
    bt.x_dtype = OFFSIM_F32;
    bt.dO = net->layers_host[0].in;
    PpoNet N;
    PpoBatchArgs B;
    size_t lds;
    int rc = ppou_prepare("ppo_update_work_doubles_pop", net, OFFSIM_PPO_ACTOR, &bt, N, B, lds);  // (any last width up to 16: a critic's too)
    if (rc) return rc;
    B.M = M;
    const unsigned nb = ppou_blocks(B);
    return (int64_t)L * ppou_pop_stride(nb ? (int)nb : 1, N.P);
}

extern "C" int offsim_ppo_grad_pop(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, int32_t L, int32_t E,
                                   const double *clip_ratio, float *grad, double *stats, double *work, void *stream) {
    PpoNet N;
    PpoBatchArgs B;
    size_t lds;
    int rc = ppou_prepare_pop("ppo_grad_pop", net, kind, batch, L, E, N, B, lds);
    if (rc) return rc;
    if (!clip_ratio) return fail(OFFSIM_EINVAL, "ppo_grad_pop: clip_ratio is NULL%s");
    for (int l = 0; l < L; l++)
        if (!ppou_clip_ok(clip_ratio[l])) return fail(OFFSIM_EINVAL, "ppo_grad_pop: every clip_ratio must be in [0, 1)%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!grad || !stats || !work) return fail(OFFSIM_EINVAL, "ppo_grad_pop: grad / stats / work is NULL%s");
    hipStream_t s = (hipStream_t)stream;
    const int nb = (int)ppou_blocks(B);
    const int64_t stride = ppou_pop_stride(nb, N.P);
    rc = ppou_pop_init(L, nullptr, clip_ratio, nullptr, work, stride, 8 * nb, s);
    if (rc) return rc;
    rc = ppou_launch_grad<true>(kind, batch->x_dtype, N, B, lds, work, s, L);
    if (rc) return rc;
    PpoAdamArgs O;
    memset(&O, 0, sizeof(O));
    O.stats = stats;
    O.grad_out = grad;
    O.kind = kind;
    O.nblocks = nb;
    hipLaunchKernelGGL((k_ppo_adam<false, true>), dim3((N.P + PPOU_ADAM_BLOCK - 1) / PPOU_ADAM_BLOCK, (unsigned)L), dim3(PPOU_ADAM_BLOCK), 0, s, N, O,
                       work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_ppo_update_pop(const offsim_ppo_net *net, int32_t kind, const offsim_ppo_batch *batch, int32_t L, int32_t E,
                                     const double *clip_ratio, const double *target_kl, int32_t iters, const offsim_ppo_adam_pop *opt, double *stats,
                                     double *trace, double *work, void *stream) {
    PpoNet N;
    PpoBatchArgs B;
    size_t lds;
    int rc = ppou_prepare_pop("ppo_update_pop", net, kind, batch, L, E, N, B, lds);
    if (rc) return rc;
    if (!clip_ratio || !target_kl || !opt || !opt->lr) return fail(OFFSIM_EINVAL, "ppo_update_pop: clip_ratio / target_kl / opt / opt->lr is NULL%s");
    for (int l = 0; l < L; l++) {
        if (!ppou_clip_ok(clip_ratio[l])) return fail(OFFSIM_EINVAL, "ppo_update_pop: every clip_ratio must be in [0, 1)%s");
        if (!(target_kl[l] >= 0.0)) return fail(OFFSIM_EINVAL, "ppo_update_pop: every target_kl must be >= 0%s");
        if (!(opt->lr[l] >= 0.0)) return fail(OFFSIM_EINVAL, "ppo_update_pop: every lr must be >= 0%s");
    }
    if (iters < 0) return fail(OFFSIM_EINVAL, "ppo_update_pop: iters must be >= 0%s");
    if (B.M == 0 || iters == 0) return OFFSIM_OK;
    if (!opt->m || !opt->v || !opt->t) return fail(OFFSIM_EINVAL, "ppo_update_pop: opt->m / v / t is NULL%s");
    if (!stats || !trace || !work) return fail(OFFSIM_EINVAL, "ppo_update_pop: stats / trace / work is NULL%s");
    hipStream_t s = (hipStream_t)stream;
    const int nb = (int)ppou_blocks(B);
    const int64_t stride = ppou_pop_stride(nb, N.P);
    rc = ppou_pop_init(L, opt->lr, clip_ratio, target_kl, work, stride, 8 * nb, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(trace, 0xff, (size_t)L * iters * 2 * sizeof(double), s));  // passes that never ran stay NaN
    PpoAdamArgs O;
    memset(&O, 0, sizeof(O));
    O.m = opt->m;
    O.v = opt->v;
    O.t = opt->t;
    O.stats = stats;
    O.trace = trace;
    O.kind = kind;
    O.nblocks = nb;
    O.iters = iters;
    const dim3 agrid((N.P + PPOU_ADAM_BLOCK - 1) / PPOU_ADAM_BLOCK, (unsigned)L);
    for (int i = 0; i < iters; i++) {
        rc = ppou_launch_grad<true>(kind, batch->x_dtype, N, B, lds, work, s, L);
        if (rc) return rc;
        O.iter = i;
        hipLaunchKernelGGL((k_ppo_adam<true, true>), agrid, dim3(PPOU_ADAM_BLOCK), 0, s, N, O, work);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ppo_finish_pop, dim3((L + 255) / 256), dim3(256), 0, s, opt->t, (const double *)stats, (const double *)work, (int)iters, (int)L,
                       stride, 8 * nb);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}
