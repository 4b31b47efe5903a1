// HOMER encoder training on the device (include/offsim.h: offsim_homer_grad, offsim_homer_step; HOMEREncoder.train / loss_grad): one
// batch of offsim4rl/encoders/homer.py:81-91 -- _calc_loss, backward, clip_grad_norm_, Adam -- as three launches, with the Gumbel
// noise and the batch indices as inputs.
//
//   k_homer_grad<XT, BWD>  one fused forward, loss and backward pass over M records.  A workgroup of 512 threads stages the four layers'
//                          W^T and b into LDS once (pmlp_stage, the padded W^T stride of k_ppo_grad) and takes tiles of TM records
//                          (tile i of workgroup b is b + i * gridDim.x).  A tile lives in LDS in two row spaces:
//                            encoder rows    r = s * TM + m, s = 0 obs[i], 1 next_obs[i], 2 next_obs[j]:
//                                            Ae [3 TM][x (dO) | h (H) | 1],  De [3 TM][dh (H) | e, then de (nZ)]
//                            classifier rows r = c * TM + m, c = 0 real, 1 impostor:
//                                            Ac [2 TM][z_a (nZ) | onehot (nA) | z_b (nZ) | h (H) | 1],  Dc [2 TM][dh (H) | logits, then d (2) | dx (2 nZ + nA)]
//                          Phases per tile, a __syncthreads between them: load, encoder forward (2 layers), the four Gumbel softmaxes
//                          (thread = one z vector), classifier forward (2 layers), loss and output delta (thread = classifier row),
//                          and with BWD: classifier backward (2 layers), softmax backward into de (thread = encoder row; the prev row
//                          sums z0's and z2's), encoder backward, then G: every thread adds the tile's sum_m D[m][j] A[m][k] to each
//                          parameter it owns (p = tid + 512 i, in registers for the whole launch), the encoder's over 3 TM rows, the
//                          classifier's over 2 TM.  Invalid records and the tail of the last tile get zero inputs, zero noise and a zero
//                          output delta.  At the end: the partial gradient (f32 [P]) and the partial sums of n and -log p (f64) to scratch.
//   k_homer_reduce<STEP>   thread = parameter: the partials summed in block order in f64, / (2 n), rounded to f32 (the gradient: what
//                          offsim_homer_grad returns), its square reduced per block in a fixed tree.  STEP: block 0 also moves Adam's t.
//   k_homer_adam           every block sums the blocks' squares in the same order -> total_norm, coef; then one thread per parameter:
//                          clip, weight decay, Adam (k_ppo_adam's arithmetic), in place.
// No float atomics, no cooperative launch, nothing waits on another workgroup.
//
// A population (offsim_homer_grad_pop, offsim_homer_step_pop; the POP instances of the same three kernels) puts L independent encoders
// on gridDim.y.  Learner l = blockIdx.y has the stacked network l (pmlp_stage's lrn; k_homer_adam steps W + l * out * in, b + l * out),
// its own records (idx_real / idx_impo at l * idx_stride + m, noise at (l * idx_stride + m) * 4 * nZ) over the shared obs / next_obs /
// act, its own scratch block (ht_pop_stride: sized by the nb workgroups a learner really has), its own lr / weight_decay /
// max_grad_norm (f64 device arrays) and its own rows of grad, m, v, t and stats.  Every launch of row l reads active[l] first and
// returns when it is 0.  Per learner TM, the tiles of a workgroup, the partials, the reduction order, the norm tree and Adam are the
// single call's on the same M, so learner l's results are the single call's bit for bit.  The POP = false instances carry none of this.
#pragma once

#define HT_THREADS 512
#define HT_OWN (OFFSIM_HOMER_MAX_FLOATS / HT_THREADS)  // parameters per thread
#define HT_RB 4                                         // rows per thread in the forward and backward layer products
#define HT_RED_BLOCK 256
static_assert(HT_OWN * HT_THREADS >= OFFSIM_HOMER_MAX_FLOATS, "every parameter needs an owner");

struct HomerNet {
    float *W[4];  // 0, 1: obs_encoder.0 / .2; 2, 3: classifier.0 / .2
    float *b[4];
    int in[4], out[4], goff[4], woff[4], boff[4], ldw[4];  // goff: flat offset of the layer's W (b follows); LDS: W^T [in][ldw], b [out]
    int n;                                                  // 4 (pmlp_stage's layer count)
    int dO, nA, nZ, H, K, P, w_floats;                      // K = 2 nZ + nA
    int lda_e, ldd_e, lda_c, ldd_c;
    float slope;
};

struct HomerBatchArgs {
    const void *obs, *next_obs;
    const int32_t *act, *idx_real, *idx_impo;
    const float *noise;
    int64_t n_rows, M;
    int TM, hard;
    float tau;
    int64_t idx_stride;     // POP: the learner stride of idx_real / idx_impo / noise, in records
    const uint8_t *active;  // POP: [L] or NULL (all active)
};

// scratch (doubles): [NB][2] partial (n, sum -log p) | 8 spare | squares [ceil(P / 256)] | gradient f32 [P] | partials f32 [NB][P], with
// NB = OFFSIM_HOMER_MAX_BLOCKS for the single call; POP: one such block per learner, NB = the nb workgroups a learner really has
__host__ __device__ __forceinline__ int ht_nred(int P) { return (P + HT_RED_BLOCK - 1) / HT_RED_BLOCK; }
__host__ __device__ __forceinline__ size_t ht_pop_stride(int nb, int P) { return OFFSIM_HOMER_WORK_DOUBLES_NB(P, nb); }
template <bool POP>
__host__ __device__ __forceinline__ size_t ht_sq(int nb) {
    return (size_t)(POP ? nb : OFFSIM_HOMER_MAX_BLOCKS) * 2 + 8;
}
template <bool POP>
__host__ __device__ __forceinline__ size_t ht_gflat(int nb, int P) {
    return ht_sq<POP>(nb) + ht_nred(P);
}
template <bool POP>
__host__ __device__ __forceinline__ size_t ht_gpart(int nb, int P) {
    return ht_gflat<POP>(nb, P) + (P + 1) / 2;
}

// y[r][j] = act?(sum_k x[r][k] W^T[k][j] + b[j]) for R rows (a multiple of HT_RB): thread = (HT_RB rows, one unit), one fmaf chain per row
__device__ __forceinline__ void ht_layer_fwd(const float *x, int ldx, float *y, int ldy, const float *wt, int ldw, const float *bias, int in, int out, int R,
                                             bool act, float slope, int tid) {
    for (int e = tid; e < (R / HT_RB) * out; e += HT_THREADS) {
        const int mb = e / out, j = e - mb * out;
        const float *x0 = x + (size_t)(HT_RB * mb) * ldx;
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
        for (int k = 0; k < in; k++) {
            const float w = wt[k * ldw + j];
            c0 = fmaf(x0[k], w, c0);
            c1 = fmaf(x0[ldx + k], w, c1);
            c2 = fmaf(x0[2 * ldx + k], w, c2);
            c3 = fmaf(x0[3 * ldx + k], w, c3);
        }
        const float bj = bias[j];
        float *y0 = y + (size_t)(HT_RB * mb) * ldy + j;
        y0[0] = act ? pmlp_act(c0 + bj, OFFSIM_ACT_LEAKY_RELU, slope) : c0 + bj;
        y0[ldy] = act ? pmlp_act(c1 + bj, OFFSIM_ACT_LEAKY_RELU, slope) : c1 + bj;
        y0[2 * ldy] = act ? pmlp_act(c2 + bj, OFFSIM_ACT_LEAKY_RELU, slope) : c2 + bj;
        y0[3 * ldy] = act ? pmlp_act(c3 + bj, OFFSIM_ACT_LEAKY_RELU, slope) : c3 + bj;
    }
}

// dp[r][k] = (sum_j dn[r][j] W^T[k][j]) * (h ? leaky_relu'(h[r][k]) : 1): thread = (HT_RB rows, one input unit)
__device__ __forceinline__ void ht_layer_bwd(const float *dn, int ldn, float *dp, int ldp, const float *wt, int ldw, const float *h, int ldh, int in, int out,
                                             int R, float slope, int tid) {
    for (int e = tid; e < (R / HT_RB) * in; e += HT_THREADS) {
        const int mb = e / in, k = e - mb * in;
        const float *d0 = dn + (size_t)(HT_RB * mb) * ldn;
        const float *wk = wt + k * ldw;
        float c[HT_RB] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < out; j++) {
            const float w = wk[j];
            c[0] = fmaf(d0[j], w, c[0]);
            c[1] = fmaf(d0[ldn + j], w, c[1]);
            c[2] = fmaf(d0[2 * ldn + j], w, c[2]);
            c[3] = fmaf(d0[3 * ldn + j], w, c[3]);
        }
        float *p0 = dp + (size_t)(HT_RB * mb) * ldp + k;
#pragma unroll
        for (int q = 0; q < HT_RB; q++) {
            const float s = h ? (h[(size_t)(HT_RB * mb + q) * ldh + k] > 0.0f ? 1.0f : slope) : 1.0f;
            p0[q * ldp] = c[q] * s;
        }
    }
}

template <typename XT, bool BWD, bool POP = false>
__global__ void __launch_bounds__(HT_THREADS) k_homer_grad(HomerNet N, HomerBatchArgs B, double *__restrict__ work) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int lrn = POP ? (int)blockIdx.y : 0;
    if constexpr (POP) {  // the learner's records and scratch; a quiet learner's workgroups leave before the first barrier
        if (B.active && !B.active[lrn]) return;
        work += (size_t)lrn * ht_pop_stride((int)gridDim.x, N.P);
        B.idx_real += (int64_t)lrn * B.idx_stride;
        B.idx_impo += (int64_t)lrn * B.idx_stride;
        if (B.noise) B.noise += (int64_t)lrn * B.idx_stride * 4 * N.nZ;
    }
    const int tid = threadIdx.x, TM = B.TM, dO = N.dO, nA = N.nA, nZ = N.nZ, H = N.H, K = N.K;
    const int lda_e = N.lda_e, ldd_e = N.ldd_e, lda_c = N.lda_c, ldd_c = N.ldd_c;
    float *w_lds = (float *)lds_raw;
    float *Ae = w_lds + N.w_floats;
    float *De = Ae + (size_t)3 * TM * lda_e;
    float *Ac = De + (size_t)3 * TM * ldd_e;
    float *Dc = Ac + (size_t)2 * TM * lda_c;
    int *rec = (int *)(Dc + (size_t)2 * TM * ldd_c);  // [3][TM]: i, j, act (act < 0: the record is invalid)
    double *red = (double *)(rec + 4 * TM);            // [2 TM][2]  (all sizes above are multiples of 2 floats: ld* odd times TM even)

    pmlp_stage(w_lds, N, N.ldw, tid, HT_THREADS, lrn);
    for (int e = tid; e < 3 * TM * lda_e; e += HT_THREADS) Ae[e] = 0.0f;
    for (int e = tid; e < 3 * TM * ldd_e; e += HT_THREADS) De[e] = 0.0f;
    for (int e = tid; e < 2 * TM * lda_c; e += HT_THREADS) Ac[e] = 0.0f;
    for (int e = tid; e < 2 * TM * ldd_c; e += HT_THREADS) Dc[e] = 0.0f;
    __syncthreads();
    for (int r = tid; r < 3 * TM; r += HT_THREADS) Ae[r * lda_e + dO + H] = 1.0f;
    for (int r = tid; r < 2 * TM; r += HT_THREADS) Ac[r * lda_c + K + H] = 1.0f;

    // the parameters this thread owns: p = tid + HT_THREADS * i -> (space, D column, A column) packed
    uint32_t own[BWD ? HT_OWN : 1];
    float g[BWD ? HT_OWN : 1];
    if constexpr (BWD) {
#pragma unroll
        for (int i = 0; i < HT_OWN; i++) {
            g[i] = 0.0f;
            own[i] = 0xffffffffu;
            const int p = tid + HT_THREADS * i;
            if (p < N.P) {
                int l = 0;
                while (l + 1 < 4 && p >= N.goff[l + 1]) l++;
                const int e = p - N.goff[l], nw = N.in[l] * N.out[l];
                const int j = e < nw ? e / N.in[l] : e - nw;
                const int kk = e < nw ? e - j * N.in[l] : -1;  // -1: the bias, its A column the ones
                // D columns: De [dh | de], Dc [dh | d | dx];  A columns: Ae [x | h | 1], Ac [C | h | 1]
                const int dc = (l == 0 || l == 2) ? j : H + j;
                const int ac = (l == 0 || l == 2) ? (kk < 0 ? (l == 0 ? dO + H : K + H) : kk) : (kk < 0 ? (l == 1 ? dO + H : K + H) : (l == 1 ? dO : K) + kk);
                own[i] = ((uint32_t)(l >= 2) << 31) | ((uint32_t)dc << 16) | (uint32_t)ac;
            }
        }
    }
    const int nown = (N.P + HT_THREADS - 1) / HT_THREADS;
    double s_n = 0.0, s_loss = 0.0;  // of the classifier rows this thread is the loss thread of

    const float *wt1 = w_lds + N.woff[0], *wt2 = w_lds + N.woff[1], *wt3 = w_lds + N.woff[2], *wt4 = w_lds + N.woff[3];
    const float *bb1 = w_lds + N.boff[0], *bb2 = w_lds + N.boff[1], *bb3 = w_lds + N.boff[2], *bb4 = w_lds + N.boff[3];
    const int64_t ntiles = (B.M + TM - 1) / TM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t m0 = tile * TM;
        const int tm = (int)(B.M - m0 < TM ? B.M - m0 : TM);
        if (tid < TM) {
            int i = 0, j = 0, a = -1;
            if (tid < tm) {
                i = B.idx_real[m0 + tid];
                j = B.idx_impo[m0 + tid];
                if (i >= 0 && i < B.n_rows && j >= 0 && j < B.n_rows) {
                    a = B.act[i];
                    if (a >= nA) a = -1;
                }
            }
            rec[tid] = i;
            rec[TM + tid] = j;
            rec[2 * TM + tid] = a;
        }
        __syncthreads();
        // the tile's observations (zeros for an invalid record and past the end) and the one-hot of the action
        for (int e = tid; e < 3 * TM * dO; e += HT_THREADS) {
            const int r = e / dO, k = e - r * dO, s = r / TM, m = r - s * TM;
            float v = 0.0f;
            if (rec[2 * TM + m] >= 0) {
                const int64_t row = s == 2 ? rec[TM + m] : rec[m];
                v = pmlp_in<XT>((const XT *)(s == 0 ? B.obs : B.next_obs), row * dO + k);
            }
            Ae[r * lda_e + k] = v;
        }
        for (int e = tid; e < 2 * TM * nA; e += HT_THREADS) {
            const int r = e / nA, k = e - r * nA, m = r % TM;
            Ac[r * lda_c + nZ + k] = rec[2 * TM + m] == k ? 1.0f : 0.0f;
        }
        __syncthreads();
        // encoder forward: h = leaky_relu(x W1^T + b1) into Ae, e = h W2^T + b2 into De's de columns
        ht_layer_fwd(Ae, lda_e, Ae + dO, lda_e, wt1, N.ldw[0], bb1, dO, H, 3 * TM, true, N.slope, tid);
        __syncthreads();
        ht_layer_fwd(Ae + dO, lda_e, De + H, ldd_e, wt2, N.ldw[1], bb2, H, nZ, 3 * TM, false, N.slope, tid);
        __syncthreads();
        // z_q = softmax((e + g_q) / tau), q = 0: prev -> real's z_a, 1: real -> real's z_b, 2: prev -> impostor's z_a, 3: impostor -> impostor's z_b
        for (int e = tid; e < 4 * TM; e += HT_THREADS) {
            const int q = e / TM, m = e - q * TM;
            const float *ev = De + (size_t)((q == 0 || q == 2 ? 0 : (q == 1 ? 1 : 2)) * TM + m) * ldd_e + H;
            float *z = Ac + (size_t)((q >> 1) * TM + m) * lda_c + ((q & 1) ? nZ + nA : 0);
            const float *gn = (B.noise && rec[2 * TM + m] >= 0) ? B.noise + ((m0 + m) * 4 + q) * (int64_t)nZ : nullptr;
            float mx = -INFINITY;
            int arg = 0;
            for (int k = 0; k < nZ; k++) {
                const float u = (ev[k] + (gn ? gn[k] : 0.0f)) / B.tau;
                z[k] = u;
                if (u > mx) {
                    mx = u;
                    arg = k;
                }
            }
            float sum = 0.0f;
            for (int k = 0; k < nZ; k++) {
                const float x = expf(z[k] - mx);
                z[k] = x;
                sum = sum + x;
            }
            for (int k = 0; k < nZ; k++) {
                const float y = z[k] / sum;
                z[k] = B.hard ? ((k == arg ? 1.0f : 0.0f) - y) + y : y;
            }
        }
        __syncthreads();
        // classifier forward: h into Ac, logits into Dc's d columns
        ht_layer_fwd(Ac, lda_c, Ac + K, lda_c, wt3, N.ldw[2], bb3, K, H, 2 * TM, true, N.slope, tid);
        __syncthreads();
        ht_layer_fwd(Ac + K, lda_c, Dc + H, ldd_c, wt4, N.ldw[3], bb4, H, 2, 2 * TM, false, N.slope, tid);
        __syncthreads();
        // loss: -log_softmax(logits)[1] for the real row, [0] for the impostor row; the delta at the logits (unnormalised: / (2 n) at the end)
        if (tid < 2 * TM) {
            const int c = tid / TM, m = tid - c * TM;
            float *d = Dc + (size_t)tid * ldd_c + H;
            if (rec[2 * TM + m] < 0) {
                d[0] = d[1] = 0.0f;
            } else {
                const float z0 = d[0], z1 = d[1];
                const float mx = z1 > z0 ? z1 : z0;
                const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
                const float sum = e0 + e1;
                const float lse = mx + logf(sum);
                const int t = c == 0 ? 1 : 0;
                s_loss += (double)(-((t ? z1 : z0) - lse));
                if (c == 0) s_n += 1.0;
                d[0] = e0 / sum - (t == 0 ? 1.0f : 0.0f);
                d[1] = e1 / sum - (t == 1 ? 1.0f : 0.0f);
            }
        }
        __syncthreads();
        if constexpr (BWD) {
            // classifier backward: dh = (d W4) * act'(h), dx = dh W3
            ht_layer_bwd(Dc + H, ldd_c, Dc, ldd_c, wt4, N.ldw[3], Ac + K, lda_c, H, 2, 2 * TM, N.slope, tid);
            __syncthreads();
            ht_layer_bwd(Dc, ldd_c, Dc + H + 2, ldd_c, wt3, N.ldw[2], nullptr, 0, K, H, 2 * TM, N.slope, tid);
            __syncthreads();
            // softmax backward: de = z * (dz - sum_k dz_k z_k) / tau; the prev row (s = 0) takes z0's and z2's
            for (int r = tid; r < 3 * TM; r += HT_THREADS) {
                const int s = r / TM, m = r - s * TM;
                float *de = De + (size_t)r * ldd_e + H;
                for (int k = 0; k < nZ; k++) de[k] = 0.0f;
                for (int c = 0; c < 2; c++) {
                    if (s == 1 && c == 1) continue;  // real: z1 of the real row
                    if (s == 2 && c == 0) continue;  // impostor: z3 of the impostor row
                    const int off = s == 0 ? 0 : nZ + nA;
                    const float *z = Ac + (size_t)(c * TM + m) * lda_c + off;
                    const float *dz = Dc + (size_t)(c * TM + m) * ldd_c + H + 2 + off;
                    float dot = 0.0f;
                    for (int k = 0; k < nZ; k++) dot = fmaf(dz[k], z[k], dot);
                    for (int k = 0; k < nZ; k++) de[k] = de[k] + (z[k] * (dz[k] - dot)) / B.tau;
                }
            }
            __syncthreads();
            // encoder backward: dh = (de W2) * act'(h)
            ht_layer_bwd(De + H, ldd_e, De, ldd_e, wt2, N.ldw[1], Ae + dO, lda_e, H, nZ, 3 * TM, N.slope, tid);
            __syncthreads();
            // G
#pragma unroll
            for (int i = 0; i < HT_OWN; i++) {
                asm volatile("" : "+v"(own[i]));  // opaque per tile: the decoded pointers and strides of 40 parameters are not kept live across tiles
                if (i < nown && own[i] != 0xffffffffu) {
                    const bool cls = (own[i] >> 31) != 0u;
                    const int ldd = cls ? ldd_c : ldd_e, lda = cls ? lda_c : lda_e, R = (cls ? 2 : 3) * TM;
                    const float *dc = (cls ? Dc : De) + ((own[i] >> 16) & 0x7fffu), *ac = (cls ? Ac : Ae) + (own[i] & 0xffffu);
                    float c = 0.0f;
                    for (int r = 0; r < R; r++) c = fmaf(dc[(size_t)r * ldd], ac[(size_t)r * lda], c);
                    g[i] = g[i] + c;
                }
            }
            __syncthreads();
        }
    }
    if constexpr (BWD) {
        float *gpart = (float *)(work + ht_gpart<POP>((int)gridDim.x, N.P)) + (size_t)blockIdx.x * N.P;
#pragma unroll
        for (int i = 0; i < HT_OWN; i++) {
            const int p = tid + HT_THREADS * i;
            if (p < N.P) gpart[p] = g[i];
        }
    }
    if (tid < 2 * TM) {
        red[tid * 2 + 0] = s_n;
        red[tid * 2 + 1] = s_loss;
    }
    __syncthreads();
    if (tid < 2) {
        double s = 0.0;
        for (int r = 0; r < 2 * TM; r++) s += red[r * 2 + tid];
        work[(size_t)blockIdx.x * 2 + tid] = s;
    }
}

struct HomerOptArgs {
    float *m, *v;
    int64_t *t;
    double lr, weight_decay, max_norm;
    double *stats;
    float *grad_out;
    int nblocks, bwd;
    // POP: [L] device arrays, the width of a stats row, and the active bytes ([L] or NULL)
    const double *lr_p, *weight_decay_p, *max_norm_p;
    const uint8_t *active;
    int stats_ld;
};

// the batch's n and mean loss from the workgroups' partial sums, the same way in every block that asks
__device__ __forceinline__ void ht_sums(const double *work, int nblocks, double &n, double &loss) {
    double sn = 0.0, sl = 0.0;
    for (int b = 0; b < nblocks; b++) {
        sn += work[(size_t)b * 2];
        sl += work[(size_t)b * 2 + 1];
    }
    n = sn;
    loss = sn > 0.0 ? sl / (2.0 * sn) : 0.0;
}

template <bool STEP, bool POP = false>
__global__ void __launch_bounds__(HT_RED_BLOCK) k_homer_reduce(HomerNet N, HomerOptArgs O, double *__restrict__ work) {
    __shared__ double sq[HT_RED_BLOCK];
    __shared__ double sh[2];
    if constexpr (POP) {  // the learner's scratch and rows of the outputs and of the step count
        const int lrn = (int)blockIdx.y;
        if (O.active && !O.active[lrn]) return;
        work += (size_t)lrn * ht_pop_stride(O.nblocks, N.P);
        O.stats += (size_t)lrn * O.stats_ld;
        if (STEP) O.t += lrn;
        if (O.grad_out) O.grad_out += (size_t)lrn * N.P;
    }
    if (threadIdx.x == 0) ht_sums(work, O.nblocks, sh[0], sh[1]);
    __syncthreads();
    const double n = sh[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        O.stats[0] = n;
        O.stats[1] = sh[1];
        if (STEP && n > 0.0) *O.t += 1;  // (k_homer_adam, the next launch, reads the new count)
    }
    if (!O.bwd) return;
    const int p = blockIdx.x * HT_RED_BLOCK + threadIdx.x;
    float gf = 0.0f;
    if (p < N.P) {
        const float *gpart = (const float *)(work + ht_gpart<POP>(O.nblocks, N.P));
        double gs = 0.0;
        for (int b = 0; b < O.nblocks; b++) gs += (double)gpart[(size_t)b * N.P + p];
        gf = (float)(n > 0.0 ? gs / (2.0 * n) : 0.0);
        ((float *)(work + ht_gflat<POP>(O.nblocks, N.P)))[p] = gf;
        if (O.grad_out) O.grad_out[p] = gf;
    }
    sq[threadIdx.x] = (double)gf * (double)gf;
    __syncthreads();
    for (int s = HT_RED_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sq[threadIdx.x] += sq[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) work[ht_sq<POP>(O.nblocks) + blockIdx.x] = sq[0];
}

template <bool POP = false>
__global__ void __launch_bounds__(HT_RED_BLOCK) k_homer_adam(HomerNet N, HomerOptArgs O, double *__restrict__ work) {
    __shared__ double sh[2];
    const int lrn = POP ? (int)blockIdx.y : 0;
    if constexpr (POP) {  // the learner's scratch, hyperparameters and rows of the outputs and of the optimiser state
        if (O.active && !O.active[lrn]) return;
        work += (size_t)lrn * ht_pop_stride(O.nblocks, N.P);
        O.stats += (size_t)lrn * O.stats_ld;
        O.m += (size_t)lrn * N.P;
        O.v += (size_t)lrn * N.P;
        O.t += lrn;
        O.lr = O.lr_p[lrn];
        O.weight_decay = O.weight_decay_p[lrn];
        O.max_norm = O.max_norm_p[lrn];
    }
    if (threadIdx.x == 0) {
        double n, loss, s = 0.0;
        ht_sums(work, O.nblocks, n, loss);
        const int nr = ht_nred(N.P);
        for (int b = 0; b < nr; b++) s += work[ht_sq<POP>(O.nblocks) + b];
        sh[0] = n;
        sh[1] = sqrt(s);
    }
    __syncthreads();
    const double n = sh[0], total = sh[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) O.stats[2] = total;
    if (!(n > 0.0)) return;  // no valid record: nothing changes
    const int p = blockIdx.x * HT_RED_BLOCK + threadIdx.x;
    if (p >= N.P) return;
    // torch.nn.utils.clip_grad_norm_: every gradient is multiplied by the clamped coefficient, 1 included
    const double cc = O.max_norm / (total + 1e-6);
    const double coef = cc < 1.0 ? cc : 1.0;
    int l = 0;
    while (l + 1 < 4 && p >= N.goff[l + 1]) l++;
    const int e = p - N.goff[l], nw = N.in[l] * N.out[l];
    float *q = e < nw ? N.W[l] + (size_t)lrn * nw + e : N.b[l] + (size_t)lrn * N.out[l] + (e - nw);
    // torch.optim.Adam with L2 weight decay: b1 = 0.9, b2 = 0.999, eps = 1e-8; f64 arithmetic on the f32 state (k_ppo_adam's)
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double t = (double)*O.t;
    const double gd = (double)((const float *)(work + ht_gflat<POP>(O.nblocks, N.P)))[p] * coef + O.weight_decay * (double)*q;
    const float mf = (float)(b1 * (double)O.m[p] + (1.0 - b1) * gd);
    const float vf = (float)(b2 * (double)O.v[p] + (1.0 - b2) * gd * gd);
    const double step = O.lr / (1.0 - pow(b1, t));
    const double den = sqrt((double)vf) / sqrt(1.0 - pow(b2, t)) + eps;
    O.m[p] = mf;
    O.v[p] = vf;
    *q = (float)((double)*q - step * (double)mf / den);
}

static int ht_check_net(const char *who, const offsim_homer_net *net, int &P) {
    if (!net) return fail(OFFSIM_EINVAL, "%s: net is NULL", who);
    if (!net->enc_W1 || !net->enc_b1 || !net->enc_W2 || !net->enc_b2 || !net->cls_W1 || !net->cls_b1 || !net->cls_W2 || !net->cls_b2)
        return fail(OFFSIM_EINVAL, "%s: a weight or bias pointer of the net is NULL", who);
    if (net->dO < 1 || net->dO > PMLP_MAX_IN) return fail(OFFSIM_EINVAL, "%s: observation width must be 1..128", who);
    if (net->H < 1 || net->H > PMLP_MAX_HIDDEN) return fail(OFFSIM_EINVAL, "%s: hidden width must be 1..256", who);
    if (net->nZ < 2 || net->nZ > 256) return fail(OFFSIM_EINVAL, "%s: nZ must be 2..256", who);
    if (net->nA < 1 || net->nA > PMLP_MAX_ACTIONS) return fail(OFFSIM_EINVAL, "%s: nA must be 1..16", who);
    if (!(net->slope >= 0.0f)) return fail(OFFSIM_EINVAL, "%s: a leaky_relu slope below 0 is not supported", who);
    const int K = 2 * net->nZ + net->nA;
    P = net->dO * net->H + net->H + net->H * net->nZ + net->nZ + K * net->H + net->H + 2 * net->H + 2;
    return OFFSIM_OK;
}

// The net and the batch of a pass, and k_homer_grad's layouts of them.
static int ht_prepare(const char *who, const offsim_homer_net *net, const offsim_homer_batch *bt, double tau, HomerNet &N, HomerBatchArgs &B, size_t &lds) {
    int P = 0;
    int rc = ht_check_net(who, net, P);
    if (rc) return rc;
    if (!bt) return fail(OFFSIM_EINVAL, "%s: batch is NULL", who);
    if (bt->x_dtype != OFFSIM_F32 && bt->x_dtype != OFFSIM_F16) return fail(OFFSIM_EINVAL, "%s: x_dtype must be OFFSIM_F32 or OFFSIM_F16", who);
    if (!(tau > 0.0) || !((float)tau > 0.0f)) return fail(OFFSIM_EINVAL, "%s: tau must be > 0", who);
    if (bt->M < 0 || bt->n_rows < 0) return fail(OFFSIM_EINVAL, "%s: M and n_rows must be >= 0", who);
    if (bt->M > 0 && (!bt->obs || !bt->next_obs || !bt->act || !bt->idx_real || !bt->idx_impo))
        return fail(OFFSIM_EINVAL, "%s: obs / next_obs / act / idx_real / idx_impo is NULL", who);
    memset(&N, 0, sizeof(N));
    memset(&B, 0, sizeof(B));
    const int dO = net->dO, nA = net->nA, nZ = net->nZ, H = net->H, K = 2 * nZ + nA;
    float *const W[4] = {net->enc_W1, net->enc_W2, net->cls_W1, net->cls_W2};
    float *const b[4] = {net->enc_b1, net->enc_b2, net->cls_b1, net->cls_b2};
    const int in[4] = {dO, H, K, H}, out[4] = {H, nZ, H, 2};
    int goff = 0, wf = 0;
    for (int l = 0; l < 4; l++) {
        N.W[l] = W[l];
        N.b[l] = b[l];
        N.in[l] = in[l];
        N.out[l] = out[l];
        N.goff[l] = goff;
        goff += in[l] * out[l] + out[l];
        N.ldw[l] = out[l] | 1;
        N.woff[l] = wf;
        wf += in[l] * N.ldw[l];
        N.boff[l] = wf;
        wf += out[l];
    }
    if (P > OFFSIM_HOMER_MAX_FLOATS) return fail(OFFSIM_EUNSUPPORTED, "%s: the two networks' parameters exceed OFFSIM_HOMER_MAX_FLOATS", who);
    N.n = 4;
    N.dO = dO;
    N.nA = nA;
    N.nZ = nZ;
    N.H = H;
    N.K = K;
    N.P = P;
    N.slope = net->slope;
    N.w_floats = (wf + 3) & ~3;
    N.lda_e = (dO + H + 1) | 1;
    N.ldd_e = (H + nZ) | 1;
    N.lda_c = (K + H + 1) | 1;
    N.ldd_c = (H + 2 + K) | 1;
    int TM = 32;
    for (;; TM /= 2) {
        lds = sizeof(float) * ((size_t)N.w_floats + (size_t)TM * (3 * (N.lda_e + N.ldd_e) + 2 * (N.lda_c + N.ldd_c)) + 4 * (size_t)TM) + sizeof(double) * 4 * TM;
        if (lds <= 160 * 1024 || TM == HT_RB) break;
    }
    if (lds > 160 * 1024) return fail(OFFSIM_EUNSUPPORTED, "%s: the weights and one tile's activations exceed 160 KiB of LDS", who);
    // a small batch is latency-bound: smaller tiles spread it over more workgroups (the tile is a function of the shapes and M alone)
    while (TM > 8 && bt->M < (int64_t)TM * 8) {
        TM /= 2;
        lds = sizeof(float) * ((size_t)N.w_floats + (size_t)TM * (3 * (N.lda_e + N.ldd_e) + 2 * (N.lda_c + N.ldd_c)) + 4 * (size_t)TM) + sizeof(double) * 4 * TM;
    }
    B.obs = bt->obs;
    B.next_obs = bt->next_obs;
    B.act = bt->act;
    B.idx_real = bt->idx_real;
    B.idx_impo = bt->idx_impo;
    B.noise = bt->noise;
    B.n_rows = bt->n_rows;
    B.M = bt->M;
    B.TM = TM;
    B.tau = (float)tau;
    return OFFSIM_OK;
}

static unsigned ht_blocks(const HomerBatchArgs &B) {
    const int64_t nt = (B.M + B.TM - 1) / B.TM;
    return (unsigned)(nt < OFFSIM_HOMER_MAX_BLOCKS ? nt : OFFSIM_HOMER_MAX_BLOCKS);
}

// POP: L learners on gridDim.y (B.M: one learner's records)
template <bool POP = false>
static int ht_launch_grad(int32_t x_dtype, bool bwd, const HomerNet &N, const HomerBatchArgs &B, size_t lds, double *work, hipStream_t s, int L = 1) {
    dim3 grid(ht_blocks(B), (unsigned)L), block(HT_THREADS);
#define LAUNCH_HT(XT, BWD)                                                                      \
    do {                                                                                        \
        if (lds > 64 * 1024) HIP_TRY(allow_big_lds((k_homer_grad<XT, BWD, POP>), (int)lds));    \
        hipLaunchKernelGGL((k_homer_grad<XT, BWD, POP>), grid, block, lds, s, N, B, work);      \
    } while (0)
    if (x_dtype == OFFSIM_F32) {
        if (bwd) LAUNCH_HT(float, true);
        else LAUNCH_HT(float, false);
    } else {
        if (bwd) LAUNCH_HT(__half, true);
        else LAUNCH_HT(__half, false);
    }
#undef LAUNCH_HT
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int64_t offsim_homer_work_doubles(const offsim_homer_net *net) {
    int P = 0;
    int rc = ht_check_net("homer_work_doubles", net, P);
    if (rc) return rc;
    return OFFSIM_HOMER_WORK_DOUBLES(P);
}

extern "C" int offsim_homer_grad(const offsim_homer_net *net, const offsim_homer_batch *batch, double tau, int32_t hard, float *grad, double *stats,
                                 double *work, void *stream) {
    HomerNet N;
    HomerBatchArgs B;
    size_t lds;
    int rc = ht_prepare("homer_grad", net, batch, tau, N, B, lds);
    if (rc) return rc;
    if (hard && grad) return fail(OFFSIM_EINVAL, "homer_grad: hard is forward only: grad must be NULL%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!stats || !work) return fail(OFFSIM_EINVAL, "homer_grad: stats / work is NULL%s");
    B.hard = hard ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    rc = ht_launch_grad(batch->x_dtype, grad != nullptr, N, B, lds, work, s);
    if (rc) return rc;
    HomerOptArgs O;
    memset(&O, 0, sizeof(O));
    O.stats = stats;
    O.grad_out = grad;
    O.nblocks = (int)ht_blocks(B);
    O.bwd = grad != nullptr;
    hipLaunchKernelGGL((k_homer_reduce<false>), dim3(O.bwd ? ht_nred(N.P) : 1), dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_homer_step(const offsim_homer_net *net, const offsim_homer_batch *batch, double tau, double max_grad_norm,
                                 const offsim_homer_adam *adam, double *stats, double *work, void *stream) {
    HomerNet N;
    HomerBatchArgs B;
    size_t lds;
    int rc = ht_prepare("homer_step", net, batch, tau, N, B, lds);
    if (rc) return rc;
    if (!(max_grad_norm >= 0.0)) return fail(OFFSIM_EINVAL, "homer_step: max_grad_norm must be >= 0%s");
    if (!adam || !(adam->lr >= 0.0) || !(adam->weight_decay >= 0.0)) return fail(OFFSIM_EINVAL, "homer_step: adam is NULL or its lr / weight_decay is negative%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!adam->m || !adam->v || !adam->t) return fail(OFFSIM_EINVAL, "homer_step: adam->m / v / t is NULL%s");
    if (!stats || !work) return fail(OFFSIM_EINVAL, "homer_step: stats / work is NULL%s");
    hipStream_t s = (hipStream_t)stream;
    rc = ht_launch_grad(batch->x_dtype, true, N, B, lds, work, s);
    if (rc) return rc;
    HomerOptArgs O;
    memset(&O, 0, sizeof(O));
    O.m = adam->m;
    O.v = adam->v;
    O.t = adam->t;
    O.lr = adam->lr;
    O.weight_decay = adam->weight_decay;
    O.max_norm = max_grad_norm;
    O.stats = stats;
    O.nblocks = (int)ht_blocks(B);
    O.bwd = 1;
    const dim3 grid(ht_nred(N.P));
    hipLaunchKernelGGL((k_homer_reduce<true>), grid, dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((k_homer_adam<false>), grid, dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

// ---- a population of L encoders (include/offsim.h: offsim_homer_grad_pop, offsim_homer_step_pop) ----

// ht_prepare for a population: B describes ONE learner's M records, of the [L, idx_stride] arrays
static int ht_prepare_pop(const char *who, const offsim_homer_net *net, const offsim_homer_batch_pop *bt, int32_t L, double tau, HomerNet &N,
                          HomerBatchArgs &B, size_t &lds) {
    if (L <= 0 || L > 65535) return fail(OFFSIM_EINVAL, "%s: L must be in 1..65535", who);
    if (!bt) return fail(OFFSIM_EINVAL, "%s: batch is NULL", who);
    if (bt->M >= 0 && bt->idx_stride < bt->M) return fail(OFFSIM_EINVAL, "%s: idx_stride must be >= M", who);
    offsim_homer_batch one;
    memset(&one, 0, sizeof(one));
    one.obs = bt->obs;
    one.next_obs = bt->next_obs;
    one.x_dtype = bt->x_dtype;
    one.act = bt->act;
    one.n_rows = bt->n_rows;
    one.idx_real = bt->idx_real;
    one.idx_impo = bt->idx_impo;
    one.noise = bt->noise;
    one.M = bt->M;
    int rc = ht_prepare(who, net, &one, tau, N, B, lds);
    if (rc) return rc;
    B.idx_stride = bt->idx_stride;
    return OFFSIM_OK;
}

extern "C" int64_t offsim_homer_work_doubles_pop(const offsim_homer_net *net, int32_t L, int64_t M) {
    if (L <= 0 || M < 0) return fail(OFFSIM_EINVAL, "homer_work_doubles_pop: L must be >= 1 and M >= 0%s");
    // ht_prepare's TM for M records: every M from 32 * OFFSIM_HOMER_MAX_BLOCKS on has the same TM and OFFSIM_HOMER_MAX_BLOCKS workgroups
    offsim_homer_batch bt;
    memset(&bt, 0, sizeof(bt));
    bt.x_dtype = OFFSIM_F32;
    bt.M = M < (int64_t)32 * OFFSIM_HOMER_MAX_BLOCKS ? M : (int64_t)32 * OFFSIM_HOMER_MAX_BLOCKS;
    bt.obs = bt.next_obs = &bt;  // (never read: ht_prepare only refuses NULL)
    bt.act = bt.idx_real = bt.idx_impo = (const int32_t *)&bt;
    HomerNet N;
    HomerBatchArgs B;
    size_t lds;
    int rc = ht_prepare("homer_work_doubles_pop", net, &bt, 1.0, N, B, lds);
    if (rc) return rc;
    const unsigned nb = ht_blocks(B);
    return (int64_t)L * (int64_t)ht_pop_stride(nb ? (int)nb : 1, N.P);
}

extern "C" int offsim_homer_grad_pop(const offsim_homer_net *net, const offsim_homer_batch_pop *batch, int32_t L, double tau, int32_t hard,
                                     const uint8_t *active, float *grad, double *stats, double *work, void *stream) {
    HomerNet N;
    HomerBatchArgs B;
    size_t lds;
    int rc = ht_prepare_pop("homer_grad_pop", net, batch, L, tau, N, B, lds);
    if (rc) return rc;
    if (hard && grad) return fail(OFFSIM_EINVAL, "homer_grad_pop: hard is forward only: grad must be NULL%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!stats || !work) return fail(OFFSIM_EINVAL, "homer_grad_pop: stats / work is NULL%s");
    B.hard = hard ? 1 : 0;
    B.active = active;
    hipStream_t s = (hipStream_t)stream;
    rc = ht_launch_grad<true>(batch->x_dtype, grad != nullptr, N, B, lds, work, s, L);
    if (rc) return rc;
    HomerOptArgs O;
    memset(&O, 0, sizeof(O));
    O.stats = stats;
    O.stats_ld = 2;
    O.grad_out = grad;
    O.nblocks = (int)ht_blocks(B);
    O.bwd = grad != nullptr;
    O.active = active;
    hipLaunchKernelGGL((k_homer_reduce<false, true>), dim3(O.bwd ? ht_nred(N.P) : 1, (unsigned)L), dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}

extern "C" int offsim_homer_step_pop(const offsim_homer_net *net, const offsim_homer_batch_pop *batch, int32_t L, double tau,
                                     const offsim_homer_adam_pop *adam, const uint8_t *active, double *stats, double *work, void *stream) {
    HomerNet N;
    HomerBatchArgs B;
    size_t lds;
    int rc = ht_prepare_pop("homer_step_pop", net, batch, L, tau, N, B, lds);
    if (rc) return rc;
    if (!adam) return fail(OFFSIM_EINVAL, "homer_step_pop: adam is NULL%s");
    if (B.M == 0) return OFFSIM_OK;
    if (!adam->m || !adam->v || !adam->t) return fail(OFFSIM_EINVAL, "homer_step_pop: adam->m / v / t is NULL%s");
    if (!adam->lr || !adam->weight_decay || !adam->max_grad_norm)
        return fail(OFFSIM_EINVAL, "homer_step_pop: adam->lr / weight_decay / max_grad_norm is NULL%s");
    if (!stats || !work) return fail(OFFSIM_EINVAL, "homer_step_pop: stats / work is NULL%s");
    B.active = active;
    hipStream_t s = (hipStream_t)stream;
    rc = ht_launch_grad<true>(batch->x_dtype, true, N, B, lds, work, s, L);
    if (rc) return rc;
    HomerOptArgs O;
    memset(&O, 0, sizeof(O));
    O.m = adam->m;
    O.v = adam->v;
    O.t = adam->t;
    O.lr_p = adam->lr;
    O.weight_decay_p = adam->weight_decay;
    O.max_norm_p = adam->max_grad_norm;
    O.stats = stats;
    O.stats_ld = 3;
    O.nblocks = (int)ht_blocks(B);
    O.bwd = 1;
    O.active = active;
    const dim3 grid(ht_nred(N.P), (unsigned)L);
    hipLaunchKernelGGL((k_homer_reduce<true, true>), grid, dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((k_homer_adam<true>), grid, dim3(HT_RED_BLOCK), 0, s, N, O, work);
    LAUNCH_CHECK();
    return OFFSIM_OK;
}
