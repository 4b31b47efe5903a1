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
        case OFFSIM_ACT_RELU: return v > 0.0f ? v : 0.0f;
        case OFFSIM_ACT_LEAKY_RELU: return v > 0.0f ? v : v * slope;  // torch: x if x > 0 else slope * x
        default: return v;
    }
}

// One output unit of a layer: sum_k x[k] * w[k * ws] as ONE fmaf chain in k order, then + bias (b NULL: none), then the activation unless
// the layer is the last.  Shared by k_policy_mlp (w = a row of W, ws = 1) and the in-wave forward of offsim_vector_collect (w = a column
// of W^T, ws = out), so both produce the same bits.
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

// VALUE: the critic of the same shape (offsim_value_mlp, spinup's MLPCritic: v = squeeze(v_net(obs), -1)): the last layer has one unit and
// no softmax follows, probs is then out[M].
template <typename XT, bool VALUE>
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
        const float *__restrict__ W = L.W[l];
        const float *__restrict__ b = L.b[l];
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
    for (int m = threadIdx.x; m < tm; m += blockDim.x) pmlp_softmax(cur + m * ld, nA, probs + (m0 + m) * nA);
}

static size_t policy_mlp_lds_bytes(const PmlpLayers &L) { return sizeof(float) * (2 * (size_t)PMLP_TM * (L.w_max + 1) + (size_t)L.w_floats); }
