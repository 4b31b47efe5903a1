// Policy MLP forward for the row-policy evalMC (include/offsim.h: offsim_policy_mlp): probs[m] = softmax(L_n(act(... act(L_1(x[rows[m]])))))
// -- spinup's MLPCategoricalActor (offsim4rl/agents/ppo.py:18-27: logits_net = Linear -> act -> ... -> Linear, Categorical(logits).probs).
//
// VALU, f32 throughout: every output is ONE fmaf chain over the layer's inputs in k order, then + bias (x @ W^T + b).  The forward is a
// small part of a row-policy evaluation (one pass over the log against a scan of millions of steps per rollout, tools/bench_obs_policy.py),
// so the kernel is written for clarity and bounded LDS, not for the matrix cores.
//
// One workgroup of 256 threads = a tile of PMLP_TM rows.  The tile's activations live in LDS in two ping-pong buffers [PMLP_TM][w_max + 1]
// (+1: rows fall on different banks); every layer's weights are staged into LDS in chunks of output rows ([jc][in + 1], at most
// PMLP_W_FLOATS floats), so a layer of any supported size goes through the same loop.  The last layer's logits go through a max-subtracted
// softmax, one thread per row, in the order torch's softmax reduces (max, then the sum of exp(x - max) left to right).
#pragma once

#define PMLP_TM 32                 // rows per workgroup
#define PMLP_W_FLOATS (64 * 257)   // LDS floats for one chunk of a layer's weights
#define PMLP_MAX_LAYERS 4
#define PMLP_MAX_IN 128            // observation width
#define PMLP_MAX_HIDDEN 256
#define PMLP_MAX_ACTIONS 16

// THE description of a network on the host: what offsim_policy_mlp / offsim_value_mlp, offsim_vector_collect[_ppo] (actor and critic) and
// offsim_ppo_grad / offsim_ppo_update all take.  pmlp_describe is the only place that knows the limits; each entry point derives its own
// kernel's descriptor (LDS layout, chunk size, parameter offsets) from this.
struct PmlpNet {
    const float *W[PMLP_MAX_LAYERS];
    const float *b[PMLP_MAX_LAYERS];  // NULL: no bias
    int in[PMLP_MAX_LAYERS], out[PMLP_MAX_LAYERS];
    int n, act, dO, w_max;  // number of layers, OFFSIM_ACT_*, observation width, widest activation (input included)
    float slope;
};

#define PMLP_OUT_ACTIONS 0  // pmlp_describe's n_out: the last layer has 1..16 units (an actor's logits)

// Validates a network (1-4 Linear layers, f32 / f16 observations of width 1..128, a known activation, W present, widths that chain, hidden
// widths <= 256, and the last layer: n_out units -- 1 for a critic, a table's nA -- or PMLP_OUT_ACTIONS) and fills N.  LAYER:
// offsim_mlp_layer or offsim_ppo_layer (the same layout with writable pointers).  `who` names the entry point in the error text.
template <typename LAYER>
static int pmlp_describe(const char *who, const LAYER *layers_host, int n, int dO, int activation, float slope, int x_dtype, int n_out, PmlpNet &N) {
    if (!layers_host || n < 1 || n > PMLP_MAX_LAYERS) return fail(OFFSIM_EINVAL, "%s: 1 to 4 Linear layers", who);
    if (x_dtype != OFFSIM_F32 && x_dtype != OFFSIM_F16) return fail(OFFSIM_EINVAL, "%s: x_dtype must be OFFSIM_F32 or OFFSIM_F16", who);
    if (activation != OFFSIM_ACT_IDENTITY && activation != OFFSIM_ACT_TANH && activation != OFFSIM_ACT_RELU && activation != OFFSIM_ACT_LEAKY_RELU)
        return fail(OFFSIM_EINVAL, "%s: unknown activation", who);
    if (dO < 1 || dO > PMLP_MAX_IN) return fail(OFFSIM_EINVAL, "%s: observation width must be 1..128", who);
    N = PmlpNet{};
    N.n = n;
    N.act = activation;
    N.slope = slope;
    N.dO = N.w_max = dO;
    for (int l = 0; l < n; l++) {
        const LAYER &y = layers_host[l];
        const bool last = l == n - 1;
        if (!y.W) return fail(OFFSIM_EINVAL, "%s: a layer's W is NULL", who);
        if (y.in != (l == 0 ? dO : layers_host[l - 1].out)) return fail(OFFSIM_EINVAL, "%s: layer widths do not chain", who);
        if (last && n_out == 1 && y.out != 1) return fail(OFFSIM_EINVAL, "%s: the last layer must have one output unit", who);
        if (y.out < 1 || y.out > (last ? PMLP_MAX_ACTIONS : PMLP_MAX_HIDDEN))
            return fail(OFFSIM_EINVAL, last ? "%s: more than 16 actions" : "%s: hidden width above 256", who);
        if (last && n_out != PMLP_OUT_ACTIONS && y.out != n_out) return fail(OFFSIM_EINVAL, "%s: the network's outputs differ from the table's nA", who);
        N.W[l] = y.W;
        N.b[l] = y.b;
        N.in[l] = y.in;
        N.out[l] = y.out;
        if (y.out > N.w_max) N.w_max = y.out;
    }
    return OFFSIM_OK;
}

// k_policy_mlp's descriptor
struct PmlpLayers {
    const float *W[PMLP_MAX_LAYERS];
    const float *b[PMLP_MAX_LAYERS];
    int in[PMLP_MAX_LAYERS], out[PMLP_MAX_LAYERS];
    int n, w_max;  // number of layers, widest activation (input included)
    int w_floats;  // LDS floats for a chunk of weights: the largest layer's out * (in + 1), at most PMLP_W_FLOATS
};

__device__ __forceinline__ float pmlp_act(float v, int act, float slope) {
    switch (act) {
        case OFFSIM_ACT_TANH: return tanhf(v);
        case OFFSIM_ACT_RELU: return !(v <= 0.0f) ? v : 0.0f;  // torch: NaN stays NaN (the NaN row of an index outside x, include/offsim.h)
        case OFFSIM_ACT_LEAKY_RELU: return v > 0.0f ? v : v * slope;  // torch: x if x > 0 else slope * x
        default: return v;
    }
}

// One output unit of a layer: sum_k x[k] * w[k * ws] as ONE fmaf chain in k order, then + bias (b NULL: none), then the activation unless
// the layer is the last.  Shared by k_policy_mlp (w = a row of W, ws = 1) and k_collect's in-wave forward (collect.hpp: collect_forward,
// w = a column of W^T, ws = out), so both produce the same bits.
__device__ __forceinline__ float pmlp_unit(const float *x, const float *w, int ws, int in, const float *b, bool last, int act, float slope) {
    float acc = 0.0f;
    for (int k = 0; k < in; k++) acc = fmaf(x[k], w[k * ws], acc);
    if (b) acc = acc + *b;
    return last ? acc : pmlp_act(acc, act, slope);
}

// softmax of the logits z[0..nA) (torch.distributions.Categorical(logits=...).probs): max-subtracted, exp, the sum left to right, one
// division per action.  One thread per row.
__device__ __forceinline__ void pmlp_softmax(const float *z, int nA, float *o) {
    float mx = z[0];
    for (int a = 1; a < nA; a++) mx = z[a] > mx ? z[a] : mx;
    float e[PMLP_MAX_ACTIONS], s = 0.0f;
    for (int a = 0; a < PMLP_MAX_ACTIONS; a++) {
        if (a < nA) {
            e[a] = expf(z[a] - mx);
            s = s + e[a];
        }
    }
    for (int a = 0; a < PMLP_MAX_ACTIONS; a++)
        if (a < nA) o[a] = e[a] / s;
}

// log of the probability of action a under the logits z[0..nA) (torch.distributions.Categorical(logits=...).log_prob(a), which
// normalises by logsumexp = max + log(sum(exp(z - max)))): z[a] - (max + logf(sum)), the max and the sum in pmlp_softmax's order.  One
// thread per row (the PPO buffer's logp, offsim_vector_collect_ppo).
__device__ __forceinline__ float pmlp_logp(const float *z, int nA, int a) {
    float mx = z[0];
    for (int b = 1; b < nA; b++) mx = z[b] > mx ? z[b] : mx;
    float s = 0.0f;
    for (int b = 0; b < nA; b++) s = s + expf(z[b] - mx);
    return z[a] - (mx + logf(s));
}

template <typename XT>
__device__ __forceinline__ float pmlp_in(const XT *x, int64_t i);
template <>
__device__ __forceinline__ float pmlp_in<float>(const float *x, int64_t i) { return x[i]; }
template <>
__device__ __forceinline__ float pmlp_in<__half>(const __half *x, int64_t i) { return __half2float(x[i]); }

// Stages a network for a kernel that keeps all of it in LDS (k_collect, k_ppo_grad), all nt threads of the workgroup striding: per layer
// W [out][in] (read coalesced) -> W^T [in][ld[l]] at dst + woff[l], then b at dst + boff[l] (boff < 0: no bias).  N: that kernel's
// descriptor, with W, b, in, out, woff, boff and n; nt: the workgroup's size as that kernel has it (blockDim.x, or its constant).
// lrn: which network of a stacked population (W [L][out][in], b [L][out]; the descriptor is learner 0's); 0 for a single network.
template <typename NET, typename NT>
__device__ __forceinline__ void pmlp_stage(float *dst, const NET &N, const int *ld, int tid, NT nt, int lrn = 0) {
    for (int l = 0; l < N.n; l++) {
        const int in = N.in[l], out = N.out[l], ldw = ld[l];
        const float *__restrict__ W = N.W[l] + (size_t)lrn * in * out;
        for (int e = tid; e < in * out; e += nt) {
            const int j = e / in, k = e - j * in;
            dst[N.woff[l] + k * ldw + j] = W[e];
        }
        if (N.boff[l] >= 0)
            for (int j = tid; j < out; j += nt) dst[N.boff[l] + j] = N.b[l][(size_t)lrn * out + j];
    }
}

// VALUE: the critic of the same shape (offsim_value_mlp, spinup's MLPCritic: v = squeeze(v_net(obs), -1)): the last layer has one unit and
// no softmax follows, probs is then out[M].
// POP: a stacked population (offsim_policy_mlp_pop: W [L][out][in], b [L][out], L's descriptor is learner 0's), the learner is blockIdx.y:
// the same tile loop on that learner's tensors, written to probs [L][M][nA].
template <typename XT, bool VALUE, bool POP = false>
__global__ void __launch_bounds__(256) k_policy_mlp(const XT *__restrict__ x, int64_t n_x, int dO, const int32_t *__restrict__ rows, int64_t M,
                                                    PmlpLayers L, int act, float slope, float *__restrict__ probs) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int ld = L.w_max + 1;
    float *buf0 = (float *)lds_raw, *buf1 = buf0 + PMLP_TM * ld, *wl = buf1 + PMLP_TM * ld;
    const int64_t m0 = (int64_t)blockIdx.x * PMLP_TM;
    const int tm = (int)(M - m0 < PMLP_TM ? M - m0 : PMLP_TM);
    // row m of the tile: x[rows[m0 + m]] (an index outside [0, n_x) gives NaN probabilities instead of a read out of bounds)
    for (int e = threadIdx.x; e < tm * dO; e += blockDim.x) {
        const int m = e / dO, k = e - m * dO;
        const int64_t src = rows ? (int64_t)rows[m0 + m] : m0 + m;
        buf0[m * ld + k] = (src >= 0 && src < n_x) ? pmlp_in<XT>(x, src * dO + k) : __builtin_nanf("");
    }
    float *cur = buf0, *nxt = buf1;
    for (int l = 0; l < L.n; l++) {
        const int in = L.in[l], out = L.out[l], ldw = in + 1;
        const int jc_max = L.w_floats / ldw;
        const float *__restrict__ W = L.W[l] + (POP ? (size_t)blockIdx.y * in * out : 0);
        const float *__restrict__ b = POP && L.b[l] ? L.b[l] + (size_t)blockIdx.y * out : L.b[l];
        const bool last = l == L.n - 1;
        for (int j0 = 0; j0 < out; j0 += jc_max) {
            const int jc = out - j0 < jc_max ? out - j0 : jc_max;
            __syncthreads();  // (the previous chunk's readers are done with wl; the tile's inputs are written)
            for (int e = threadIdx.x; e < jc * in; e += blockDim.x) {
                const int j = e / in, k = e - j * in;
                wl[j * ldw + k] = W[(int64_t)(j0 + j) * in + k];
            }
            __syncthreads();
            for (int e = threadIdx.x; e < tm * jc; e += blockDim.x) {
                const int m = e / jc, j = e - m * jc;
                nxt[m * ld + j0 + j] = pmlp_unit(cur + m * ld, wl + j * ldw, 1, in, b ? b + j0 + j : nullptr, last, act, slope);
            }
        }
        __syncthreads();
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
    if constexpr (VALUE) {
        for (int m = threadIdx.x; m < tm; m += blockDim.x) probs[m0 + m] = cur[m * ld];
        return;
    }
    // softmax of the logits (torch.distributions.Categorical(logits=...).probs)
    const int nA = L.out[L.n - 1];
    if (POP) probs += (int64_t)blockIdx.y * M * nA;
    for (int m = threadIdx.x; m < tm; m += blockDim.x) pmlp_softmax(cur + m * ld, nA, probs + (m0 + m) * nA);
}

static size_t policy_mlp_lds_bytes(const PmlpLayers &L) { return sizeof(float) * (2 * (size_t)PMLP_TM * (L.w_max + 1) + (size_t)L.w_floats); }
