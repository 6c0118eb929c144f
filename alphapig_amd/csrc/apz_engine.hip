// libalphapig_hip.so -- C ABI (include/alphapig_hip.h) over the gfx950 kernels.
// Host-side glue only: parameter table, buffer ownership, launch sequencing on one HIP stream (the BatchNorm
// fold and weight packing kernels of weights_pack.h included), HIP-event timing hooks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "alphapig_hip.h"
#include "conv3x3_mfma.h"
#include "heads.h"
#include "trunk15_ring.h"
#include "trunk15_wino3.h"
#include "trunk15_wino3s.h"
#include "trunk15_wino3b.h"
#include "trunk15_wino3h.h"
#include "trunk15_wino3h16.h"
#include "trunk15_wino3hs.h"
#include "conv8_split.h"
#include "conv15_split.h"
#include "conv8_small.h"
#include "wgrad_wino3.h"
#include "wgrad_wino3h.h"
#include "sampler.h"
#include "conv_train.h"
#include "bn_frame.h"
#include "grad_guard.h"
#include "ema.h"
#include "heads_train.h"
#include "weights_pack.h"
#include "act_max.h"
#include "replay.h"
#include "frame15.h"
#include "leaf_sym.h"

namespace {

typedef std::lock_guard<std::recursive_mutex> EngineLock;

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(APZ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                  \
    } while (0)

constexpr double BN_EPS = 1e-3;   // MXNet BatchNorm default (policy_value_net_mxnet.py:54,78,81)

struct Param {
    std::string name;
    int64_t size;
};

struct ConvLayer {
    std::string name;       // conv parameter prefix
    std::string bn;         // BN parameter prefix
    std::string mean_sfx, var_sfx;
    bool fix_gamma;
    int cin, cin_pad, cout;
    bool residual;          // add the block input before ReLU
    // The packed forms of the layer's weights.  alloc_packed decides from the engine's configuration which of them the
    // layer has (and zeroes them: the pad slots are never written again), pack_all fills every one that is there with the
    // kernels of weights_pack.h, for apz_load_weights and apz_load_weights_dev alike.
    float* wpk = nullptr;   // direct convolution: [cot][c4][tap][lane]; trunk15_ring_kernel layers: [cot][c4][lane][12]
    float* wpk12 = nullptr; // 8x8 boards (conv8_kernel): [cot][c4][lane][12]
    float* upk2 = nullptr;  // trunk15_wino3_kernel: transformed weights G g G^T, [cot][row half][c4][lane][20] (wino_common.h)
    float* upk3s = nullptr; // trunk15_wino3s_kernel: the same values, [cot][wave][c4][piece][lane][4] (WinoPackSmall)
    void* upk3b = nullptr;  // trunk15_wino3b_kernel (apz_set_trunk_arith(APZ_ARITH_BF16X3) only): U as three bf16 terms (Wino3B)
    void* upk3h = nullptr;  // trunk15_wino3h_kernel (APZ_ARITH_F16X2 only): U S[co] as two fp16 terms (Wino3H)
    float* bias3h = nullptr;   // ... and its [128 biases][128 x 1 / S[co]]
    void* wpk8h = nullptr;  // conv8h_kernel / conv15h_kernel (8x8 boards and generic 15x15 nets, APZ_ARITH_F16X2, C_in a multiple of 64): w S[co] as two fp16 terms (Conv8H)
    float* bias8h = nullptr;   // ... and its [cout biases][cout x 1 / S[co]]
    float* bias = nullptr;
    // APZ_ARITH_F16X2, 15x15 trunk layers: the static exponent a of the layer's input scale 2^a (trunk15_wino3h16.h,
    // WINO3H16_PLAIN_SCALED); 0 = the unscaled kernel.  Engine state: weight loads do not touch it.
    int act_exp = 0;
};

struct Pending {
    int cls;
    hipEvent_t a, b;
    int launches;   // kernel launches bracketed by the pair
};

struct LdsAttr {
    const void* kernel;   // host function pointer
    int bytes;            // largest hipFuncAttributeMaxDynamicSharedMemorySize configured so far
};

// The exchange of the small-batch trunk kernels (T = apz::Wino3S, apz::Wino3HS): the workgroups that share a board meet
// through global slabs + ticket words keyed by a per-launch epoch (csrc/trunk15_wino3s.h)
template <class T>
struct TicketExchange {
    float* slabs = nullptr;        // row partials of the position halves
    unsigned* tickets = nullptr;   // the pairs' ticket words (each launch exchanges its epoch in)
    unsigned epoch = 0;            // last epoch handed out; never 0, never repeated between two memsets of the words

    // In front of every launch on `stream`: allocates at the first one and hands out the launch's epoch
    int prepare(hipStream_t stream, unsigned* launch_epoch) {
        if (!slabs) HIP_TRY(hipMalloc((void**)&slabs, T::slab_floats() * sizeof(float)));
        if (!tickets) {
            HIP_TRY(hipMalloc((void**)&tickets, T::counters() * sizeof(unsigned)));
            epoch = 0;
        }
        if (++epoch == 0 || epoch == 1) {
            // first launch, or the 32-bit epoch wrapped: zero the words ON THE LAUNCH STREAM (ordered before the kernel)
            epoch = 1;
            HIP_TRY(hipMemsetAsync(tickets, 0, T::counters() * sizeof(unsigned), stream));
        }
        *launch_epoch = epoch;
        return APZ_OK;
    }
    // apz_submit_codes captures no launch sequence this close to the wrap: the ticket reset has to stay outside a capture
    bool near_wrap() const { return epoch >= 0xFFFF0000u; }
    void release() {
        if (slabs) (void)hipFree(slabs);
        if (tickets) (void)hipFree(tickets);
        slabs = nullptr;
        tickets = nullptr;
    }
};

// A device buffer that grows on demand: the training entry points' scratch.  Growth waits for the device first (whatever
// still reads the old block was queued by an earlier call), and a failed allocation leaves the buffer empty, not stale.
struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;

    int reserve(size_t need) {
        if (need <= bytes) return APZ_OK;
        HIP_TRY(hipDeviceSynchronize());
        if (ptr) HIP_TRY(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        HIP_TRY(hipMalloc(&ptr, need));
        bytes = need;
        return APZ_OK;
    }
    template <class T>
    T* as() const { return (T*)ptr; }
    operator void*() const { return ptr; }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

}  // namespace

struct apz_engine {
    apz_config cfg;
    int hw = 0, code_stride = 0, num_cu = 256, cmax = 0, clast = 0;
    hipStream_t stream = nullptr;
    std::vector<Param> params;
    std::vector<ConvLayer> convs;
    bool loaded = false;
    // heads
    float *w6 = nullptr, *b6 = nullptr, *wfc_pk = nullptr, *bfc = nullptr, *wv = nullptr, *bv = nullptr;
    // device buffers
    float* act[3] = {nullptr, nullptr, nullptr};
    float *planes = nullptr, *featp = nullptr, *featv = nullptr, *probs = nullptr, *values = nullptr, *fc_logits = nullptr;
    unsigned char* codes = nullptr;
    int *perm_s = nullptr, *perm_p = nullptr;
    // apz_set_leaf_symmetry (csrc/leaf_sym.h): what forward_codes_sym puts around forward_from_codes.  APZ_SYM_NONE: nothing.
    int sym_mode = APZ_SYM_NONE;
    uint64_t sym_seed = 0;
    // apz_set_legal_policy: the heads take their softmax over the empty cells of each board.  The occupancy is the code bytes
    // of the forward where it was given codes (the heads read them in place); a forward given planes stages it in `occ`.
    bool legal_policy = false;
    unsigned char* occ = nullptr;            // [max_batch][hw], allocated by the first call that turns the switch on
    int* perm_pinv = nullptr;                // [8][hw]: perm_pinv[k][perm_p[k][p]] = p, uploaded by the first call that turns a mode on
    // the forward's own input and output under a mode: the image codes, the head's answers on them and the boards' keys --
    // one set per submission slot + one for the synchronous entry points (index APZ_MAX_SLOTS), allocated at first use,
    // max_batch rows each.  Never e->codes / e->probs / e->values, which the entry points themselves stage through.
    struct SymStage {
        unsigned char *codes = nullptr, *k = nullptr;
        float *probs = nullptr, *values = nullptr;
    } sym[APZ_MAX_SLOTS + 1];
    // host pinned staging (apz_forward_host)
    float *h_planes = nullptr, *h_probs = nullptr, *h_values = nullptr;
    unsigned char* h_codes = nullptr;
    int last_n = 0;
    // stream-ordered submission slots (apz_submit_codes / apz_wait)
    struct Slot {
        unsigned char* h_codes = nullptr;
        float *h_probs = nullptr, *h_values = nullptr;
        float *d_probs = nullptr, *d_values = nullptr;
        unsigned char* d_codes = nullptr;
        hipEvent_t done = nullptr;
        int n = 0;
        bool busy = false;
    } slots[APZ_MAX_SLOTS];
    // One lock for everything that touches the engine's buffers, stream, weights or timing state.  Recursive: the
    // public entry points call each other (apz_forward_codes_host -> _async -> apz_encode_planes).  The pipeline
    // workers of SelfPlayEngine submit from their own threads while the main thread may call policy_value_fn,
    // set_params or the arena -- every such call now queues behind the submissions instead of racing them.
    // apz_submit_codes: the forward of a small batch is tens of launches (one board on the 10-block net: 45), each a few
    // microseconds of host time -- the third submission of a (slot, batch size) pair captures the launch sequence into a
    // HIP graph (the slot's code / result buffers and the engine's activation buffers are fixed addresses) and later ones
    // replay it with one call.  Dropped whenever the weights or the kernel selection change.  OFF by default
    // (apz_set_forward_graphs): measured on ROCm 7.2 / MI355X (tools/graph_ab.py, profiles/r04_graph_ab.log) the replay is
    // SLOWER than the plain launches -- BASELINE config 2 (seven launches per 32-board forward) 337 k -> 310 k leaf
    // evaluations/s, one-board policy_value_fn (45 launches) 0.332 -> 0.338 ms.
    std::map<long, hipGraphExec_t> fwd_graphs;
    std::map<long, int> fwd_seen;
    bool use_graphs = false;
    std::recursive_mutex submit_lock;
    bool ring = false;      // 15x15 / 128-filter resnet: trunk activations in rows16 layout (trunk15_ring.h)
    bool small8 = false;    // 8x8 boards: conv8_kernel / head8_kernel (conv8_small.h)
    // Framed engines (csrc/frame15.h): a square board of side frame_s in 6..14 (not 8, not 10) in the top-left corner of the 15x15
    // frame of a `ring` engine; 0 = not framed.  hw, code_stride, the heads and the tables stay those of the S x S board.
    int frame_s = 0;
    float* fplanes = nullptr;   // framed input planes [max_batch][9][15][15]
    float* wfc_raw = nullptr;   // head8_kernel: the policy FullyConnected weight as stored, [hw][4 hw]
    int act_ps = 0, act_rs = 0;
    std::vector<LdsAttr> lds_attrs;   // need_lds: one entry per kernel launched with dynamic LDS so far
    // persistent sampler staging (apz_sample_moves_host)
    int32_t* smp_vis = nullptr;
    float* smp_pi = nullptr;
    int32_t* smp_mv = nullptr;
    uint64_t* smp_keys = nullptr;
    size_t smp_cap = 0;
    float* zeros256 = nullptr;          // bias stand-in for bias-free convolutions (ensure_zeros256)
    double* fold_ws = nullptr;                     // pack_all: scale / shift of one layer (2 x cmax doubles)
    float* stage = nullptr;                        // apz_load_weights: the host tensors, back to back in table order
    // the training entry points' scratch (train_call keeps two streams from working on it at once)
    DeviceBuffer bn_part;                          // apz_bn_fwd / _bwd: per-(channel, batch split) partial sums [256 * BN_SPLITS][2]
    DeviceBuffer wgw_scratch;                      // the weight gradients' partial sums per batch slice
    DeviceBuffer head_scratch;                     // apz_conv1x1_bwd2 / apz_bias_grad / apz_pv_loss: per-board partial sums
    DeviceBuffer adam_tab;                         // apz_adam_step: device copy of the tensor table
    DeviceBuffer guard_part;                       // apz_grad_norm / apz_adam_step_guarded: [32 ntensors] doubles, then as many words
    DeviceBuffer gather_entries;                   // apz_replay_gather: device copy of the entry words
    DeviceBuffer wino_scratch[2];                  // apz_wino_conv: rows16 input / output copies
    DeviceBuffer conv15h_scratch;                  // apz_conv15h_fwd: the call's scale / shift, bias8h and packed weights
    DeviceBuffer conv15h_tab;                      // apz_conv15h_pack_many: the step's layer table
    hipStream_t scratch_stream = nullptr;          // the stream of the last entry point that may have used the scratch buffers
    bool scratch_stream_valid = false;
    TicketExchange<apz::Wino3S> w3s;         // trunk15_wino3s_kernel
    // apz_set_trunk_uniform: APZ_ARITH_F16X2 batches of <= 32 boards run trunk15_wino3hs_kernel (the batched kernel's bits)
    bool uniform_trunk = false;
    TicketExchange<apz::Wino3HS> w3hs;       // ... and its exchange (trunk15_wino3hs.h)
    bool no_small_trunk = false;             // apz_test_select_trunk(APZ_TRUNK_WINOGRAD_BATCHED): tests compare the two forms
    bool no_quarter_trunk = false;           // apz_test_select_trunk(APZ_TRUNK_WINOGRAD_NO_QUARTER): 64-channel items for every batch
    int trunk_arith = APZ_ARITH_F32;         // apz_set_trunk_arith: APZ_ARITH_BF16X3 / _F16X2 = the split kernels for batches > 32
    // APZ_ARITH_F16X2: trunk15_wino3h_kernel raises a word when an activation left the fp16 range (a non-finite output);
    // the words live in pinned host memory, one per submission slot + one for the synchronous entry points; the entry
    // point that collects a forward's results looks at its word and repeats the forward on the exact-fp32 kernel.
    // Which word a forward raises, and everything else that holds for one forward only, is its FwdMode: not engine state.
    unsigned* ovf_host = nullptr;            // [APZ_MAX_SLOTS + 1]
    unsigned* ovf_dev = nullptr;             // the same words as the device sees them
    // APZ_ARITH_F16X2, batches > 32: trunk15_wino3h16_kernel (16-channel chunks, three products); APZ_F16X2_K8=1 in the
    // environment at engine creation selects its predecessor trunk15_wino3h_kernel instead (A/B measurements)
    bool f16x2_k8 = false;
    long ovf_repeats = 0;                    // forwards repeated so far (apz_trunk_overflows)
    // static activation exponents (apz_set_trunk_act_exponents ...): max |input| of every trunk convolution, measured by
    // act_absmax_kernel during a calibration forward or the exact repeat of an overflowed one (FwdMode::measure_max)
    bool act_auto = false;                   // apz_set_act_scale_auto: an overflow lowers the exponents
    float* amax_dev = nullptr;               // [trunk layer][ActMax::MAX_PARTS] partial maxima
    float* amax_host = nullptr;              // ... pinned copy, valid after the stream synchronisation behind the forward
    int trunk_kernel = APZ_TRUNK_WINOGRAD;   // or APZ_TRUNK_DIRECT (trunk15_ring_kernel): apz_test_select_trunk, tests only
    // profiling
    bool profiling = false;
    int prof_stride = 1, prof_phase = 0;   // time every prof_stride-th forward only
    bool prof_now = false;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    double k_ms[APZ_K_COUNT] = {0};
    long k_cnt[APZ_K_COUNT] = {0};
};

namespace {

// What holds for ONE forward (or one re-run of the trunk) and for nothing after it: built by the entry point, passed down
// to the launchers by const reference.  The persistent configuration stays in apz_engine; trunk_route() reads both.
struct FwdMode {
    unsigned* ovf = nullptr;     // (device pointer) the overflow word this forward raises; null = not armed
    bool exact = false;          // exact fp32 whatever trunk_arith: the repeat of an overflowed forward, calibration's measuring pass
    bool measure_max = false;    // max |x| in front of every trunk convolution (exact forwards only)
    bool batched = false;        // the batched form at every batch size: calibration's proving pass (or e->no_small_trunk)
    bool untimed = false;        // no event pairs whatever e->profiling says: the layer bench and the layer read-backs
};

// The mode of a forward that raises overflow word `idx` (a slot's, or APZ_MAX_SLOTS: the synchronous entry points'); other
// arithmetics than APZ_ARITH_F16X2 have no words.  Who reads the word afterwards zeroes e->ovf_host[idx] first; prewarm, the
// layer bench and the read-backs arm it too (the f16x2 kernels need one) and nobody reads what they raise.
FwdMode armed(const apz_engine* e, int idx) {
    FwdMode m;
    if (e->trunk_arith == APZ_ARITH_F16X2 && e->ovf_dev) m.ovf = e->ovf_dev + idx;
    return m;
}

void add_param(apz_engine* e, const std::string& n, int64_t sz) { e->params.push_back({n, sz}); }

void build_tables(apz_engine* e) {
    const apz_config& c = e->cfg;
    const int hw = e->hw;
    auto conv_act = [&](const std::string& name, int cin, int cout, int k) {
        add_param(e, name + "_weight", (int64_t)cout * cin * k * k);
        add_param(e, name + "_bias", cout);
        add_param(e, name + "_gamma", cout);
        add_param(e, name + "_beta", cout);
        add_param(e, name + "_mean", cout);
        add_param(e, name + "_var", cout);
    };
    int last = 0;
    if (c.net_kind == APZ_NET_RESNET) {
        const int F = c.n_filter;
        conv_act("res_conv1", c.c_in, F, 3);
        e->convs.push_back({"res_conv1", "res_conv1", "_mean", "_var", true, c.c_in, (c.c_in + 3) / 4 * 4, F, false});
        for (int i = 1; i <= c.n_blocks; i++) {
            for (const char* ab : {"A", "B"}) {
                const std::string cn = std::string("conv") + ab + std::to_string(i);
                const std::string bn = std::string("bn") + ab + std::to_string(i);
                add_param(e, cn + "_weight", (int64_t)F * F * 9);
                add_param(e, cn + "_bias", F);
                add_param(e, bn + "_gamma", F);
                add_param(e, bn + "_beta", F);
                add_param(e, bn + "_moving_mean", F);
                add_param(e, bn + "_moving_var", F);
                e->convs.push_back({cn, bn, "_moving_mean", "_moving_var", false, F, F, F, ab[0] == 'B'});
            }
        }
        last = F;
    } else {
        static const char* names[6] = {"conv1", "conv2", "conv3", "conv4", "conv5", "conv_final"};
        static const int widths[6] = {64, 64, 128, 128, 256, 256};
        int prev = c.c_in;
        for (int i = 0; i < 6; i++) {
            conv_act(names[i], prev, widths[i], 3);
            e->convs.push_back({names[i], names[i], "_mean", "_var", true, prev, (prev + 3) / 4 * 4, widths[i], false});
            prev = widths[i];
        }
        last = prev;
    }
    conv_act("conv3_1_1", last, 4, 1);
    add_param(e, "fc_3_1_1_weight", (int64_t)hw * 4 * hw);
    add_param(e, "fc_3_1_1_bias", hw);
    conv_act("conv3_2_1", last, 2, 1);
    add_param(e, "fc_3_2_1_weight", 2 * hw);
    add_param(e, "fc_3_2_1_bias", 1);
    e->clast = last;
    e->cmax = 0;
    for (auto& l : e->convs) e->cmax = std::max(e->cmax, l.cout);
}

template <typename T>
int upload(T** dst, const std::vector<T>& src) {
    if (!*dst) HIP_TRY(hipMalloc((void**)dst, src.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return APZ_OK;
}

hipEvent_t get_event(apz_engine* e) {
    if (!e->free_events.empty()) {
        hipEvent_t ev = e->free_events.back();
        e->free_events.pop_back();
        return ev;
    }
    hipEvent_t ev;
    // timing events only order work on this one device: no system-scope fence (cache write-back) when they fire
    if (hipEventCreateWithFlags(&ev, hipEventDisableSystemFence) != hipSuccess) hipEventCreate(&ev);
    return ev;
}

// `waiter` waits for everything queued on `source` so far (a pooled event; the host does not wait)
hipError_t stream_wait(apz_engine* e, hipStream_t waiter, hipStream_t source) {
    hipEvent_t ev = get_event(e);
    hipError_t he = hipEventRecord(ev, source);
    if (he == hipSuccess) he = hipStreamWaitEvent(waiter, ev, 0);
    e->free_events.push_back(ev);
    return he;
}

// Brackets one or MORE consecutive launches of one kernel class with a single event pair: an event between
// two kernels costs a barrier packet + cache maintenance (~0.1 ms each under load), so the 20 trunk launches of
// a sampled forward share one pair and their average duration is elapsed / launches.
struct Timed {
    apz_engine* e;
    int cls;
    int launches = 1;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(apz_engine* e_, int cls_, bool always = false, bool untimed = false) : e(e_), cls(cls_) {
        if (e->profiling && !untimed && (e->prof_now || always)) {
            a = get_event(e);
            b = get_event(e);
            hipEventRecord(a, e->stream);
        }
    }
    ~Timed() {
        if (a) {
            hipEventRecord(b, e->stream);
            e->pending.push_back({cls, a, b, launches});
        }
    }
};

// Recycle the pairs whose closing event has already fired (oldest first: one stream, events complete in order), so
// that a long profiled run keeps a handful of events alive instead of creating thousands.
void resolve_ready(apz_engine* e) {
    size_t k = 0;
    while (k < e->pending.size() && hipEventQuery(e->pending[k].b) == hipSuccess) {
        Pending& p = e->pending[k++];
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            e->k_ms[p.cls] += ms;
            e->k_cnt[p.cls] += p.launches;
        }
        e->free_events.push_back(p.a);
        e->free_events.push_back(p.b);
    }
    if (k) e->pending.erase(e->pending.begin(), e->pending.begin() + k);
}

void resolve_pending(apz_engine* e) {
    for (auto& p : e->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            e->k_ms[p.cls] += ms;
            e->k_cnt[p.cls] += p.launches;
        }
        e->free_events.push_back(p.a);
        e->free_events.push_back(p.b);
    }
    e->pending.clear();
}

// In front of every launch with dynamic LDS: hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel, and again
// only for a larger size.  Keyed by the kernel's host function pointer; a few dozen entries at most, searched linearly (the
// one-board forward is ~45 launches of a few microseconds each), and nothing is allocated once a kernel has its entry.
int need_lds(apz_engine* e, const void* kernel, int bytes) {
    for (LdsAttr& a : e->lds_attrs)
        if (a.kernel == kernel) {
            if (bytes > a.bytes) {
                HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
                a.bytes = bytes;
            }
            return APZ_OK;
        }
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    e->lds_attrs.push_back({kernel, bytes});
    return APZ_OK;
}

int ensure_zeros256(apz_engine* e) {
    if (!e->zeros256) {
        HIP_TRY(hipMalloc((void**)&e->zeros256, 256 * sizeof(float)));
        HIP_TRY(hipMemset(e->zeros256, 0, 256 * sizeof(float)));
    }
    return APZ_OK;
}

template <int H, int W, int CT, bool RESID>
int launch_conv_r(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n,
                  int out_ps, int out_rs, int relu = 1, int cout_groups = 1) {
    using G = apz::ConvGeo<H, W>;
    // keep channel chunks a power-of-two-ish split of Cin: 256 ch at 15x15 -> 2 x 128
    int cchunk = L.cin_pad;
    while (cchunk > G::max_chunk()) cchunk = ((cchunk / 2) + 3) & ~3;
    const int lds = G::lds_bytes(cchunk);
    auto kern = apz::conv3x3_mfma_kernel<H, W, CT, RESID>;
    // persistent grid: as many workgroups as fit at once, each loops over boards
    int per_cu = std::max(1, std::min(4, (160 * 1024) / std::max(lds, 1)));
    int grid = std::min(n, e->num_cu * per_cu);
    if (int rc = need_lds(e, (const void*)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid, cout_groups), dim3(256), lds, e->stream, in, L.wpk, L.bias, resid, out, n, L.cin,
                       L.cin_pad, cchunk, relu, out_ps, out_rs, L.cout);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

template <int H, int W, int CT>
int launch_conv_t(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    const int ps = H * W, rs = W;       // (dense planes in and out: nets with rows16 activations never come here)
    // Small batches (BASELINE config 2: 64 concurrent games = 32 boards per launch): one workgroup per board leaves most
    // CUs idle and every workgroup streams the layer's whole weight set (2.4 MB at 256 x 256) through one CU's L2 port.
    // Then each board goes to CT workgroups of 64 output channels (gridDim.y): same arithmetic per output element, in
    // the same order -- only which wave owns which channel tile changes.
    if (CT > 1 && n * CT <= 2 * e->num_cu) {
        if (resid) return launch_conv_r<H, W, 1, true>(e, L, in, resid, out, n, ps, rs, 1, CT);
        return launch_conv_r<H, W, 1, false>(e, L, in, resid, out, n, ps, rs, 1, CT);
    }
    if (resid) return launch_conv_r<H, W, CT, true>(e, L, in, resid, out, n, ps, rs);
    return launch_conv_r<H, W, CT, false>(e, L, in, resid, out, n, ps, rs);
}

template <int NW>
int launch_trunk_ring_t(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    using T = apz::Trunk15;
    const int grid = std::min(n, e->num_cu);   // one persistent workgroup per CU (LDS-bound)
    if (resid) {
        if (int rc = need_lds(e, (const void*)apz::trunk15_ring_kernel<true, NW>, T::LDS_BYTES)) return rc;
        hipLaunchKernelGGL((apz::trunk15_ring_kernel<true, NW>), dim3(grid), dim3(64 * NW), T::LDS_BYTES, e->stream, in,
                           L.wpk, L.bias, resid, out, n);
    } else {
        if (int rc = need_lds(e, (const void*)apz::trunk15_ring_kernel<false, NW>, T::LDS_BYTES)) return rc;
        hipLaunchKernelGGL((apz::trunk15_ring_kernel<false, NW>), dim3(grid), dim3(64 * NW), T::LDS_BYTES, e->stream, in,
                           L.wpk, L.bias, resid, out, n);
    }
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// trunk15_wino3_kernel addresses a launch's activations through 32-bit buffer offsets (and parks out-of-range lanes at
// offset 2^31), so one launch takes at most WINO3_MAX_BOARDS boards; larger batches go out as several launches on
// offset pointers -- a board's bits do not depend on the launch shape (tests/test_gpu_net.py).
constexpr int WINO3_MAX_BOARDS = 16384;   // even (board pairs), 16384 * 128 planes * 960 B = 2^31 - 2^27
static_assert((long long)WINO3_MAX_BOARDS * 128 * 960 < (1ll << 31), "wino3 buffer offsets");

// `launch(nb, off)` queues one launch of nb boards whose rows16 activations start `off` floats into the tensors
template <class F>
int for_board_chunks(int n, F launch) {
    using T = apz::Trunk15;
    for (int b0 = 0; b0 < n; b0 += WINO3_MAX_BOARDS)
        if (int rc = launch(std::min(n - b0, WINO3_MAX_BOARDS), (size_t)b0 * T::C * T::GPLANE)) return rc;
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

template <bool RESID, bool RELU>
int launch_wino3_t(apz_engine* e, const float* in, const float* upk, const float* bias, const float* resid, float* out, int n,
                   const float* upk_small = nullptr) {
    using T = apz::Wino3;
    if (!upk_small || n > apz::Wino3S::MAX_BOARDS || e->no_small_trunk) {
        return for_board_chunks(n, [&](int nb, size_t off) -> int {
            bool quarter = false;                                 // few pairs (training batch 128, arena): four workgroups per pair
            const int grid = apz::wino3_grid(nb, e->num_cu, e->no_quarter_trunk ? nullptr : &quarter);   // persistent workgroups; item = board pair x channel half (quarter)
            if (!quarter) {
                if (int rc = need_lds(e, (const void*)apz::trunk15_wino3_kernel<RESID, RELU>, T::LDS_BYTES)) return rc;
                hipLaunchKernelGGL((apz::trunk15_wino3_kernel<RESID, RELU>), dim3(grid), dim3(512), T::LDS_BYTES, e->stream, in + off,
                                   upk, bias, RESID ? resid + off : nullptr, out + off, nb);
            } else {
                if (int rc = need_lds(e, (const void*)apz::trunk15_wino3_kernel<RESID, RELU, true>, T::LDS_BYTES)) return rc;
                hipLaunchKernelGGL((apz::trunk15_wino3_kernel<RESID, RELU, true>), dim3(grid), dim3(512), T::LDS_BYTES, e->stream,
                                   in + off, upk, bias, RESID ? resid + off : nullptr, out + off, nb);
            }
            return APZ_OK;
        });
    }
    // the latency path: sixteen workgroups per board (16 output channels x half the positions), the same bits
    // (csrc/trunk15_wino3s.h); the halves meet through e->w3s
    unsigned epoch;
    if (int rc = e->w3s.prepare(e->stream, &epoch)) return rc;
    if (int rc = need_lds(e, (const void*)apz::trunk15_wino3s_kernel<RESID, RELU>, apz::Wino3S::LDS_BYTES)) return rc;
    hipLaunchKernelGGL((apz::trunk15_wino3s_kernel<RESID, RELU>), dim3(n * 16), dim3(256), apz::Wino3S::LDS_BYTES, e->stream, in,
                       upk_small, bias, RESID ? resid : nullptr, out, n, e->w3s.slabs, e->w3s.tickets, epoch);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// The 3 x bf16 split kernel (opt-in): same layouts, same grids, 512 threads
template <bool RESID>
int launch_wino3b_t(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    using T = apz::Wino3B;
    return for_board_chunks(n, [&](int nb, size_t off) -> int {
        const int grid = apz::wino3_grid(nb, e->num_cu);
        if (int rc = need_lds(e, (const void*)apz::trunk15_wino3b_kernel<RESID, true>, T::LDS_BYTES)) return rc;
        hipLaunchKernelGGL((apz::trunk15_wino3b_kernel<RESID, true>), dim3(grid), dim3(512), T::LDS_BYTES, e->stream, in + off,
                           (const void*)L.upk3b, L.bias, RESID ? resid + off : nullptr, out + off, nb);
        return APZ_OK;
    });
}

// The 2 x fp16 split kernels (K16: trunk15_wino3h16_kernel, else trunk15_wino3h_kernel): same layouts, same grids, 512 threads
// (SCALED, K16 only: the form with the layer's static input exponent, launched for L.act_exp != 0 and never otherwise --
// an engine without exponents runs the same code objects as before they existed)
template <bool RESID, bool K16, bool SCALED = false>
int launch_wino3h_t(apz_engine* e, const FwdMode& m, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    static_assert(K16 || !SCALED, "only the 16-channel kernel has a scaled form");
    using T = typename std::conditional<K16, apz::Wino3H16, apz::Wino3H>::type;
    constexpr int FORM = SCALED ? apz::WINO3H16_PLAIN_SCALED : apz::WINO3H16_PLAIN;
    const void* kern = K16 ? (const void*)apz::trunk15_wino3h16_kernel<RESID, true, FORM> : (const void*)apz::trunk15_wino3h_kernel<RESID, true>;
    return for_board_chunks(n, [&](int nb, size_t off) -> int {
        const int grid = apz::wino3_grid(nb, e->num_cu);
        if (int rc = need_lds(e, kern, T::LDS_BYTES)) return rc;
        if constexpr (K16)
            hipLaunchKernelGGL((apz::trunk15_wino3h16_kernel<RESID, true, FORM>), dim3(grid), dim3(512), T::LDS_BYTES, e->stream,
                               in + off, (const void*)L.upk3h, L.bias3h, RESID ? resid + off : nullptr, out + off, nb, m.ovf,
                               nullptr, SCALED ? L.act_exp : 0);
        else
            hipLaunchKernelGGL((apz::trunk15_wino3h_kernel<RESID, true>), dim3(grid), dim3(512), T::LDS_BYTES, e->stream, in + off,
                               (const void*)L.upk3h, L.bias3h, RESID ? resid + off : nullptr, out + off, nb, m.ovf);
        return APZ_OK;
    });
}

// The small-batch form of the 16-channel split kernel (apz_set_trunk_uniform): 1 .. 32 boards, eight workgroups per board,
// the batched kernel's weights, bias, overflow word and exponent -- and its bits (csrc/trunk15_wino3hs.h)
template <bool RESID, bool SCALED>
int launch_wino3hs_t(apz_engine* e, const FwdMode& m, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    using T = apz::Wino3HS;
    unsigned epoch;
    if (int rc = e->w3hs.prepare(e->stream, &epoch)) return rc;
    if (int rc = need_lds(e, (const void*)apz::trunk15_wino3hs_kernel<RESID, SCALED>, T::LDS_BYTES)) return rc;
    hipLaunchKernelGGL((apz::trunk15_wino3hs_kernel<RESID, SCALED>), dim3(T::grid(n)), dim3(512), T::LDS_BYTES, e->stream, in,
                       (const void*)L.upk3h, L.bias3h, RESID ? resid : nullptr, out, n, m.ovf, SCALED ? L.act_exp : 0,
                       e->w3hs.slabs, e->w3hs.tickets, epoch);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

template <int C4, int CIN, bool CODES>
int launch_stem15_t(apz_engine* e, const ConvLayer& L, const float* in, float* out, int n) {
    constexpr int lds = apz::stem15_lds_bytes<C4>();
    // two resident workgroups per CU; at C_in = 4 twice as many workgroups as fit, so that the dispatcher evens out the tail
    const int grid = std::min(n, e->num_cu * (C4 == 1 ? 4 : 2));
    if (int rc = need_lds(e, (const void*)apz::stem15_kernel<C4, CIN, CODES>, lds)) return rc;
    hipLaunchKernelGGL((apz::stem15_kernel<C4, CIN, CODES>), dim3(grid), dim3(256), lds, e->stream, in, L.wpk, L.bias, out, n,
                       L.cin, (int)e->code_stride);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// codes != nullptr: the stem reads the position codes itself (no planes buffer)
int launch_stem15(apz_engine* e, const ConvLayer& L, const float* in, float* out, int n, const unsigned char* codes = nullptr) {
    if (codes) {
        if (L.cin == 4) return launch_stem15_t<1, 4, true>(e, L, (const float*)codes, out, n);
        if (L.cin == 9) return launch_stem15_t<3, 9, true>(e, L, (const float*)codes, out, n);
    } else {
        if (L.cin == 4) return launch_stem15_t<1, 4, false>(e, L, in, out, n);
        if (L.cin == 9) return launch_stem15_t<3, 9, false>(e, L, in, out, n);
    }
    return fail(APZ_E_UNSUPPORTED, "stem15: C_in must be 4 or 9");
}

// 8x8 boards: work item = (board, 16 output channels), the contraction split over the four waves (conv8_small.h)
template <bool RESID, bool CODES>
int launch_conv8_t(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    using T = apz::Conv8;
    const long items = (long)n * (L.cout / 16);
    const int grid = (int)std::min<long>(items, 2L * e->num_cu);       // two workgroups per CU (LDS), persistent over items
    if (int rc = need_lds(e, (const void*)apz::conv8_kernel<RESID, CODES>, T::LDS_BYTES)) return rc;
    hipLaunchKernelGGL((apz::conv8_kernel<RESID, CODES>), dim3(grid), dim3(256), T::LDS_BYTES, e->stream, in, L.wpk12, L.bias,
                       resid, out, n, L.cin, L.cin_pad / 4, L.cout, 1, (int)e->code_stride);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// ... with split operands on the fp16 matrix pipe (conv8_split.h): same items, same grids
template <bool RESID>
int launch_conv8h_t(apz_engine* e, const FwdMode& m, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    using T = apz::Conv8H;
    const long items = (long)n * (L.cout / 16);
    const int grid = (int)std::min<long>(items, 2L * e->num_cu);
    if (int rc = need_lds(e, (const void*)apz::conv8h_kernel<RESID>, T::LDS_BYTES)) return rc;
    hipLaunchKernelGGL((apz::conv8h_kernel<RESID>), dim3(grid), dim3(256), T::LDS_BYTES, e->stream, in, (const void*)L.wpk8h,
                       L.bias8h, resid, out, n, L.cin, L.cout, 1, m.ovf);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// ... and on 15x15 boards (conv15_split.h): the same items and weights, the same rule for the grid
template <bool RESID>
int launch_conv15h_t(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n, int relu,
                     unsigned* flag) {
    using T = apz::Conv15H;
    const int grid = (int)T::grid_for((long)n * (L.cout / 16), e->num_cu);
    if (int rc = need_lds(e, (const void*)apz::conv15h_kernel<RESID>, T::LDS_BYTES)) return rc;
    hipLaunchKernelGGL((apz::conv15h_kernel<RESID>), dim3(grid), dim3(256), T::LDS_BYTES, e->stream, in, (const void*)L.wpk8h,
                       L.bias8h, resid, out, n, L.cin, L.cout, relu, flag);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

int launch_conv_generic(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n);

// The kernel of a 15x15 trunk convolution, of an 8x8 board or of a generic net's layer: DESIGN.md section 4, "Which
// arithmetic a batch gets"
enum class Route {
    F16X2_SMALL,   // trunk15_wino3hs_kernel: f16x2, <= 32 boards (apz_set_trunk_uniform)
    F16X2_K8,      // trunk15_wino3h_kernel: batched f16x2, 8-channel chunks (APZ_F16X2_K8=1)
    F16X2_K16,     // trunk15_wino3h16_kernel: batched f16x2
    BF16X3,        // trunk15_wino3b_kernel: batched bf16x3
    EXACT,         // trunk15_wino3s_kernel / trunk15_wino3_kernel: exact fp32; small, quarter or batched by launch_wino3_t
    DIRECT,        // trunk15_ring_kernel: the direct convolution, in-tree cross-check of the Winograd kernels
    CONV8H,        // conv8h_kernel: 8x8 boards, f16x2
    CONV8,         // conv8_kernel: 8x8 boards, exact fp32
    CONV15H,       // conv15h_kernel: generic 15x15 nets, f16x2
    GENERIC        // conv3x3_mfma_kernel: generic nets, exact fp32 (launch_conv_generic)
};

// (engine configuration, layer, batch size, mode) -> kernel, first match wins: the one place that decides it
Route trunk_route(const apz_engine* e, const ConvLayer& L, int n, const FwdMode& m) {
    // the f16x2 kernels raise a word: a forward without one (and the exact repeat, and a measuring pass) runs exact fp32
    const bool f16x2 = e->trunk_arith == APZ_ARITH_F16X2 && !m.exact && m.ovf;
    if (e->small8) return f16x2 && L.wpk8h ? Route::CONV8H : Route::CONV8;     // one kernel family for every batch size
    if (!e->ring) return f16x2 && L.wpk8h ? Route::CONV15H : Route::GENERIC;   // generic nets: likewise
    if (e->trunk_kernel != APZ_TRUNK_WINOGRAD || !L.upk2) return Route::DIRECT;
    const bool batched = n > apz::Wino3S::MAX_BOARDS || e->no_small_trunk || m.batched;
    if (f16x2 && L.upk3h) {
        if (batched) return e->f16x2_k8 ? Route::F16X2_K8 : Route::F16X2_K16;
        if (e->uniform_trunk && !e->f16x2_k8) return Route::F16X2_SMALL;
    }
    if (e->trunk_arith == APZ_ARITH_BF16X3 && L.upk3b && batched) return Route::BF16X3;
    return Route::EXACT;
}

// SCALED: the forms with the layer's static input exponent, F16X2_SMALL and F16X2_K16 only, launched for L.act_exp != 0 and
// never otherwise -- an engine without exponents runs the same code objects as before they existed
template <bool RESID, bool SCALED>
int launch_routed_t(apz_engine* e, const FwdMode& m, Route r, const ConvLayer& L, const float* in, const float* resid, float* out,
                    int n) {
    switch (r) {
        case Route::F16X2_SMALL: return launch_wino3hs_t<RESID, SCALED>(e, m, L, in, resid, out, n);
        case Route::F16X2_K8: return launch_wino3h_t<RESID, false>(e, m, L, in, resid, out, n);
        case Route::F16X2_K16: return launch_wino3h_t<RESID, true, SCALED>(e, m, L, in, resid, out, n);
        case Route::BF16X3: return launch_wino3b_t<RESID>(e, L, in, resid, out, n);
        case Route::EXACT: return launch_wino3_t<RESID, true>(e, in, L.upk2, L.bias, resid, out, n, m.batched ? nullptr : L.upk3s);
        case Route::DIRECT: return launch_trunk_ring_t<4>(e, L, in, resid, out, n);
        case Route::CONV8H: return launch_conv8h_t<RESID>(e, m, L, in, resid, out, n);
        case Route::CONV8: return launch_conv8_t<RESID, false>(e, L, in, resid, out, n);
        case Route::CONV15H: return launch_conv15h_t<RESID>(e, L, in, resid, out, n, 1, m.ovf);
        case Route::GENERIC: return launch_conv_generic(e, L, in, resid, out, n);
    }
}

// one convolution on the kernel of its route; resid == nullptr: no residual input
int launch_routed(apz_engine* e, const FwdMode& m, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    if (e->small8 && (L.cout % 16 || !L.wpk12)) return fail(APZ_E_UNSUPPORTED, "conv8: C_out must be a multiple of 16");
    const Route r = trunk_route(e, L, n, m);
    const bool scaled = (r == Route::F16X2_SMALL || r == Route::F16X2_K16) && L.act_exp != 0;
    if (resid) return (scaled ? launch_routed_t<true, true> : launch_routed_t<true, false>)(e, m, r, L, in, resid, out, n);
    return (scaled ? launch_routed_t<false, true> : launch_routed_t<false, false>)(e, m, r, L, in, nullptr, out, n);
}

// ---- framed engines (csrc/frame15.h)
// position codes -> e->fplanes
int launch_frame_encode(apz_engine* e, const unsigned char* codes, int n) {
    const long total = (long)n * apz::Frame15::CELLS;
    hipLaunchKernelGGL(apz::frame_encode_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 8)), dim3(256), 0,
                       e->stream, codes, e->fplanes, n, e->frame_s, e->code_stride, e->cfg.c_in);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// dense planes [n][c_in][S][S] -> e->fplanes
int launch_frame_planes(apz_engine* e, const float* planes, int n) {
    const long nplanes = (long)n * e->cfg.c_in, total = nplanes * apz::Frame15::CELLS;
    hipLaunchKernelGGL(apz::frame_planes_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 8)), dim3(256), 0,
                       e->stream, planes, e->fplanes, nplanes, e->frame_s);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// zeroes the off-board cells of the rows16 activation `act` of n boards (128 channels)
int launch_frame_clear(apz_engine* e, float* act, int n) {
    const long nplanes = (long)n * apz::Trunk15::C;            // one wavefront per plane, four per workgroup
    hipLaunchKernelGGL(apz::frame_clear_kernel, dim3((int)std::min<long>((nplanes + 3) / 4, e->num_cu * 64)), dim3(256), 0,
                       e->stream, act, nplanes, e->frame_s);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// the generic convolution (conv3x3_mfma.h): every layer of the nets that have no kernel family of their own
int launch_conv_generic(apz_engine* e, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    const int H = e->cfg.height, W = e->cfg.width, ct = L.cout / 64;
    if (H == 15 && W == 15) {
        if (ct == 2) return launch_conv_t<15, 15, 2>(e, L, in, resid, out, n);
        if (ct == 1) return launch_conv_t<15, 15, 1>(e, L, in, resid, out, n);
        if (ct == 4) return launch_conv_t<15, 15, 4>(e, L, in, resid, out, n);
    } else if (H == 8 && W == 8) {
        if (ct == 2) return launch_conv_t<8, 8, 2>(e, L, in, resid, out, n);
        if (ct == 1) return launch_conv_t<8, 8, 1>(e, L, in, resid, out, n);
        if (ct == 4) return launch_conv_t<8, 8, 4>(e, L, in, resid, out, n);
    }
    return fail(APZ_E_UNSUPPORTED, "conv3x3: unsupported board size / channel count");
}

// How the engine's first layer is queued, by the kernel family of its net
enum class FirstLayer {
    FRAMED,    // framed engines: framing kernel (from codes or dense S x S planes), the planes form of the stem, clear
    CONV8,     // 8x8 boards: conv8_kernel, which decodes position codes itself
    STEM15,    // 15x15 / 128-filter residual net: stem15_kernel, which decodes position codes itself
    GENERIC    // every other net: the generic convolution, dense planes only
};

FirstLayer first_layer(const apz_engine* e) {
    if (e->frame_s) return FirstLayer::FRAMED;
    if (e->small8) return FirstLayer::CONV8;
    return e->ring ? FirstLayer::STEM15 : FirstLayer::GENERIC;
}

// forward_from_codes: the first layer reads the position codes itself (no planes buffer)
bool stem_takes_codes(const apz_engine* e) { return first_layer(e) != FirstLayer::GENERIC; }

// layer 0 of n boards into `out`; codes != nullptr (stem_takes_codes(e) only): the position codes instead of `planes`
int launch_first_layer(apz_engine* e, const FwdMode& m, const float* planes, const unsigned char* codes, float* out, int n) {
    const ConvLayer& L = e->convs[0];
    switch (first_layer(e)) {
        case FirstLayer::FRAMED:
            if (int rc = codes ? launch_frame_encode(e, codes, n) : launch_frame_planes(e, planes, n)) return rc;
            if (int rc = launch_stem15(e, L, e->fplanes, out, n)) return rc;
            return e->convs.size() > 1 ? launch_frame_clear(e, out, n) : APZ_OK;     // (the heads read on-board cells only)
        case FirstLayer::CONV8:
            if (!codes) return launch_routed(e, m, L, planes, nullptr, out, n);
            if (L.cout % 16 || !L.wpk12) return fail(APZ_E_UNSUPPORTED, "conv8: C_out must be a multiple of 16");
            return launch_conv8_t<false, true>(e, L, (const float*)codes, nullptr, out, n);
        case FirstLayer::STEM15: return launch_stem15(e, L, planes, out, n, codes);
        case FirstLayer::GENERIC: return launch_conv_generic(e, L, planes, nullptr, out, n);
    }
}

// a layer behind the first
int launch_conv(apz_engine* e, const FwdMode& m, const ConvLayer& L, const float* in, const float* resid, float* out, int n) {
    if (int rc = launch_routed(e, m, L, in, resid, out, n)) return rc;
    // framed engines: the off-board cells zero again (skipped behind the net's last layer: the heads read on-board cells only)
    return e->frame_s && &L != &e->convs.back() ? launch_frame_clear(e, out, n) : APZ_OK;
}

// m.measure_max: max |x| of the rows16 tensor `in` (n boards, 128 channels), the input of trunk layer li >= 1, as
// partials in row li - 1 of e->amax_dev
int launch_act_max(apz_engine* e, int li, const float* in, int n) {
    const long n4 = (long)n * 128 * (apz::Trunk15::GPLANE / 4);
    float* part = e->amax_dev + (size_t)(li - 1) * apz::ActMax::MAX_PARTS;
    hipLaunchKernelGGL(apz::act_absmax_kernel, dim3(apz::ActMax::grid_for(n4)), dim3(apz::ActMax::THREADS), 0, e->stream, in, n4,
                       part);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// runs conv layers [0, upto] on `planes` (or `codes`: launch_first_layer); returns the buffer holding layer `upto`'s output
int run_trunk(apz_engine* e, const FwdMode& m, const float* planes, const unsigned char* codes, int n, int upto, float** result) {
    float *x = e->act[0], *t = e->act[1], *y = e->act[2];
    const float* cur = x;
    const int nl = (int)e->convs.size();
    const int last = std::min(upto, nl - 1);
    {
        Timed tm(e, APZ_K_STEM, false, m.untimed);       // (framed engines: the pair covers the framing kernel, the stem and its clear)
        if (int rc = launch_first_layer(e, m, planes, codes, x, n)) return rc;
    }
    if (last >= 1) {
        Timed tm(e, APZ_K_TRUNK, false, m.untimed);      // all trunk launches of this forward under one event pair
        tm.launches = last;             // (framed engines: the clears are inside the pair and counted with their layers)
        for (int li = 1; li <= last; li++) {
            const ConvLayer& L = e->convs[li];
            if (m.measure_max) {
                int rc = launch_act_max(e, li, L.residual ? t : x, n);
                if (rc) return rc;
            }
            if (e->cfg.net_kind == APZ_NET_RESNET) {
                if (!L.residual) {          // convA: x -> t
                    int rc = launch_conv(e, m, L, x, nullptr, t, n);
                    if (rc) return rc;
                    cur = t;
                } else {                    // convB: t (+x) -> y ; then y becomes the block output
                    int rc = launch_conv(e, m, L, t, x, y, n);
                    if (rc) return rc;
                    std::swap(x, y);
                    cur = x;
                }
            } else {
                float* dst = (cur == x) ? t : x;
                int rc = launch_conv(e, m, L, cur, nullptr, dst, n);
                if (rc) return rc;
                cur = dst;
            }
        }
    }
    if (m.measure_max && last >= 1)
        HIP_TRY(hipMemcpyAsync(e->amax_host, e->amax_dev, (size_t)last * apz::ActMax::MAX_PARTS * sizeof(float), hipMemcpyDeviceToHost,
                               e->stream));
    *result = const_cast<float*>(cur);
    return APZ_OK;
}

// planes [n][c_in][H][W] -> occ [n][H*W] (occupancy_planes_kernel, csrc/heads.h) on the engine's stream
int launch_occupancy_planes(apz_engine* e, const float* planes, int n, int c_in, int H, int W, unsigned char* occ) {
    const long total = (long)n * H * W;
    hipLaunchKernelGGL(apz::occupancy_planes_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 8)), dim3(256), 0,
                       e->stream, planes, occ, total, H, W, c_in);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// the heads on the trunk's output: the fused 8x8 kernel, or the two 1x1 convolutions, then the policy FullyConnected with
// softmax and value head in one launch or two.  planes / codes_dev are the forward's input, for the legal policy's mask only
int launch_heads(apz_engine* e, const float* trunk, const float* planes, const unsigned char* codes_dev, int n, float* probs,
                 float* values, float* logits, float* vlogits) {
    const int hw = e->hw;
    // legal policy: byte m of row b of `occ` is non-zero where move m is occupied -- the codes as they are, or the planes'
    // occupancy staged in e->occ (timed with the head that reads it)
    const unsigned char* occ = nullptr;
    int occ_stride = 0;
    auto stage_occupancy = [&]() -> int {
        if (!e->legal_policy) return APZ_OK;
        if (codes_dev) {
            occ = codes_dev;
            occ_stride = e->code_stride;
            return APZ_OK;
        }
        if (int rc = launch_occupancy_planes(e, planes, n, e->cfg.c_in, e->cfg.height, e->cfg.width, e->occ)) return rc;
        occ = e->occ;
        occ_stride = hw;
        return APZ_OK;
    };
    if (e->small8) {                    // both 1x1 convolutions, both FullyConnected layers, softmax and tanh in one launch
        Timed tm(e, APZ_K_HEAD_FC);
        if (int rc = stage_occupancy()) return rc;
        hipLaunchKernelGGL(occ ? apz::head8_kernel<true> : apz::head8_kernel<false>, dim3(std::min(n, e->num_cu * 8)), dim3(256), 0,
                           e->stream, trunk, e->w6, e->b6, e->wfc_raw, e->bfc, e->wv, e->bv, probs, values, logits, vlogits, n,
                           e->clast, occ, occ_stride);
        HIP_TRY(hipGetLastError());
        return APZ_OK;
    }
    {
        Timed tm(e, APZ_K_HEAD_CONV);
        if (e->ring && !e->frame_s && e->clast % 32 == 0)
            hipLaunchKernelGGL(apz::head_conv1x1_r16_kernel, dim3(n), dim3(256), 0, e->stream, trunk, e->w6, e->b6,
                               e->featp, e->featv, n, e->clast);
        else
            hipLaunchKernelGGL(apz::head_conv1x1_kernel, dim3(std::min(n, e->num_cu * 8)), dim3(256), 0, e->stream, trunk,
                               e->w6, e->b6, e->featp, e->featv, n, e->clast, hw, e->cfg.width,
                               e->ring ? e->act_ps : hw, e->ring ? e->act_rs : e->cfg.width);
        HIP_TRY(hipGetLastError());
    }
    {
        Timed tm(e, APZ_K_HEAD_FC);
        const int ntile = (hw + 15) / 16;
        const int lds = 16 * std::max(4 * hw + 1, ntile * 16) * (int)sizeof(float);
        const int grid = (n + 15) / 16;
        const int tpw = (ntile + 3) / 4;
        // (framed engines take the two-launch form at every size: at 6x6 and 7x7, hw <= 64, the fused form would be a path
        // no engine has run before; the legal policy likewise: the fused softmax has no masked form)
        if (int rc = stage_occupancy()) return rc;
        if (tpw <= 1 && !e->frame_s && !occ) {
            if (int rc = need_lds(e, (const void*)apz::head_fc_kernel<1>, lds)) return rc;
            hipLaunchKernelGGL(apz::head_fc_kernel<1>, dim3(grid), dim3(256), lds, e->stream, e->featp, e->featv,
                               e->wfc_pk, e->bfc, e->wv, e->bv, probs, values, logits, vlogits, n, hw);
        } else if (tpw <= 4) {
            // the n-tiles over four workgroups per 16 boards, then one wavefront per board for softmax + value head
            const int lds1 = 16 * (4 * hw + 1) * (int)sizeof(float);
            if (int rc = need_lds(e, (const void*)apz::head_fc_kernel<1, true>, lds1)) return rc;
            hipLaunchKernelGGL((apz::head_fc_kernel<1, true>), dim3(grid, tpw), dim3(256), lds1, e->stream, e->featp, e->featv,
                               e->wfc_pk, e->bfc, e->wv, e->bv, probs, values, logits, vlogits, n, hw, e->fc_logits);
            hipLaunchKernelGGL(occ ? apz::head_softmax_value_kernel<true> : apz::head_softmax_value_kernel<false>,
                               dim3((n + 3) / 4), dim3(256), 0, e->stream, e->fc_logits, e->featv, e->wv, e->bv, occ, occ_stride,
                               probs, values, logits, vlogits, n, hw, ntile * 16);
        } else {
            return fail(APZ_E_UNSUPPORTED, "policy head: board too large");
        }
        HIP_TRY(hipGetLastError());
    }
    return APZ_OK;
}

void drop_forward_graphs(apz_engine* e) {
    for (auto& kv : e->fwd_graphs) hipGraphExecDestroy(kv.second);
    e->fwd_graphs.clear();
    e->fwd_seen.clear();
}

// trunk, then heads.  codes_dev != nullptr (stem_takes_codes(e) only): the position codes instead of `planes`
int forward_dev(apz_engine* e, const FwdMode& m, const float* planes, const unsigned char* codes_dev, int n, float* probs,
                float* values, float* logits = nullptr, float* vlogits = nullptr) {
    if (!e->loaded) return fail(APZ_E_STATE, "weights not loaded");
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (n == 0) return APZ_OK;
    e->prof_now = e->profiling && (e->prof_phase++ % e->prof_stride == 0);
    if (e->profiling) resolve_ready(e);
    // the whole forward under one pair, EVERY forward while profiling is on: sum / wall clock = the GPU-busy fraction of a
    // measured window (two records per ~2 ms forward, at the forward's edges where the slot's `done` event sits anyway)
    Timed whole(e, APZ_K_FORWARD, true);
    float* trunk = nullptr;
    if (int rc = run_trunk(e, m, planes, codes_dev, n, (int)e->convs.size() - 1, &trunk)) return rc;
    if (int rc = launch_heads(e, trunk, planes, codes_dev, n, probs, values, logits, vlogits)) return rc;
    e->last_n = n;
    return APZ_OK;
}

// The forward of n boards from their position codes: the stem decodes them itself where it can, else they are expanded
// into e->planes first
int forward_from_codes(apz_engine* e, const FwdMode& m, const unsigned char* codes_dev, int n, float* probs, float* values) {
    if (stem_takes_codes(e)) return forward_dev(e, m, nullptr, codes_dev, n, probs, values);
    if (int rc = apz_encode_planes(e, codes_dev, n, e->cfg.c_in, e->planes)) return rc;
    return forward_dev(e, m, e->planes, nullptr, n, probs, values);
}

// mean8 runs 8 n boards in one forward: APZ_OK if the engine's buffers hold them
int sym_batch_ok(const apz_engine* e, int n) {
    if (e->sym_mode == APZ_SYM_MEAN8 && (long)n * 8 > e->cfg.max_batch)
        return fail(APZ_E_ARG, "leaf symmetry mean8 evaluates 8 boards per position: 8 * " + std::to_string(n) + " = " +
                                   std::to_string((long)n * 8) + " boards exceed max_batch = " + std::to_string(e->cfg.max_batch));
    return APZ_OK;
}

// What every entry point that forwards position codes for a caller queues: forward_from_codes, under a leaf symmetry
// between sym_expand_kernel and sym_fold_kernel (csrc/leaf_sym.h) -- the forward reads the images from, and answers into,
// staging set `stage` (a slot, or APZ_MAX_SLOTS: the synchronous entry points), and the fold writes the caller's probs /
// values.  The trunk route sees the forward's real size: n (keyed) or 8 n (mean8).  APZ_SYM_NONE: a direct call.
int forward_codes_sym(apz_engine* e, const FwdMode& m, int stage, const unsigned char* codes_dev, int n, float* probs, float* values) {
    if (e->sym_mode == APZ_SYM_NONE) return forward_from_codes(e, m, codes_dev, n, probs, values);
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (int rc = sym_batch_ok(e, n)) return rc;
    if (n == 0) return APZ_OK;
    const bool mean8 = e->sym_mode == APZ_SYM_MEAN8;
    const int images = mean8 ? 8 * n : n;
    apz_engine::SymStage& st = e->sym[stage];
    const size_t B = e->cfg.max_batch;
    if (!st.codes) HIP_TRY(hipMalloc((void**)&st.codes, B * e->code_stride));
    if (!st.probs) HIP_TRY(hipMalloc((void**)&st.probs, B * e->hw * sizeof(float)));
    if (!st.values) HIP_TRY(hipMalloc((void**)&st.values, B * sizeof(float)));
    if (!st.k) HIP_TRY(hipMalloc((void**)&st.k, B));
    {
        // (sampled profiling: forward_dev decides per forward whether its kernels are timed, so this pair follows the
        // PREVIOUS forward's decision and the fold's pair this one's; with apz_set_profiling(1) both are always timed)
        Timed tm(e, APZ_K_ENCODE, false, m.untimed);
        const dim3 grid(apz::LeafSym::expand_grid(n)), block(apz::LeafSym::THREADS);
        if (mean8)
            hipLaunchKernelGGL(apz::sym_expand_kernel<true>, grid, block, 0, e->stream, codes_dev, e->perm_p, st.codes, st.k, n,
                               e->hw, e->code_stride, e->sym_seed);
        else
            hipLaunchKernelGGL(apz::sym_expand_kernel<false>, grid, block, 0, e->stream, codes_dev, e->perm_p, st.codes, st.k, n,
                               e->hw, e->code_stride, e->sym_seed);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = forward_from_codes(e, m, st.codes, images, st.probs, st.values)) return rc;
    {
        Timed tm(e, APZ_K_ENCODE, false, m.untimed);
        const long total = (long)n * e->hw;
        const dim3 grid((int)std::min<long>((total + 255) / 256, e->num_cu * 8)), block(256);
        if (mean8)
            hipLaunchKernelGGL(apz::sym_fold_kernel<true>, grid, block, 0, e->stream, st.probs, st.values, st.k, e->perm_pinv, probs,
                               values, n, e->hw);
        else
            hipLaunchKernelGGL(apz::sym_fold_kernel<false>, grid, block, 0, e->stream, st.probs, st.values, st.k, e->perm_pinv, probs,
                               values, n, e->hw);
        HIP_TRY(hipGetLastError());
    }
    return APZ_OK;
}

// The tail of the synchronous host entry points: e->probs / e->values of n boards through the pinned staging buffers to
// the caller.  Returns with the stream drained.
int collect_to_host(apz_engine* e, int n, float* probs_host, float* values_host) {
    const size_t hw = e->hw;
    HIP_TRY(hipMemcpyAsync(e->h_probs, e->probs, n * hw * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_values, e->values, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    resolve_pending(e);
    std::memcpy(probs_host, e->h_probs, n * hw * sizeof(float));
    std::memcpy(values_host, e->h_values, n * sizeof(float));
    return APZ_OK;
}

// The head of the synchronous host entry points: the caller's planes / position codes of n boards through the pinned
// staging buffer into e->planes / e->codes, queued on the engine's stream
int stage_planes(apz_engine* e, const float* planes_host, int n) {
    const size_t bytes = (size_t)n * e->cfg.c_in * e->hw * sizeof(float);
    std::memcpy(e->h_planes, planes_host, bytes);
    HIP_TRY(hipMemcpyAsync(e->planes, e->h_planes, bytes, hipMemcpyHostToDevice, e->stream));
    return APZ_OK;
}

int stage_codes(apz_engine* e, const uint8_t* codes_host, int n) {
    const size_t bytes = (size_t)n * e->code_stride;
    std::memcpy(e->h_codes, codes_host, bytes);
    HIP_TRY(hipMemcpyAsync(e->codes, e->h_codes, bytes, hipMemcpyHostToDevice, e->stream));
    return APZ_OK;
}

// ---- static activation exponents of the f16x2 trunk kernel
// APZ_OK where they exist: the 15x15 / 128-filter residual net, APZ_ARITH_F16X2, the 16-channel kernel
int act_scale_supported(apz_engine* e) {
    if (e->small8)
        return fail(APZ_E_UNSUPPORTED, "activation exponents: the 8x8 kernels have none (conv8_split.h is in range up to 65 504)");
    if (!e->ring || e->trunk_arith != APZ_ARITH_F16X2)
        return fail(APZ_E_UNSUPPORTED, "activation exponents exist for the 15x15 / 128-filter residual net with APZ_ARITH_F16X2 only");
    if (e->f16x2_k8)
        return fail(APZ_E_UNSUPPORTED, "activation exponents: the engine was created with APZ_F16X2_K8=1, and the old kernel has no scaled form");
    return APZ_OK;
}

int act_scale_buffers(apz_engine* e) {
    const size_t bytes = (size_t)std::max<size_t>(e->convs.size() - 1, 1) * apz::ActMax::MAX_PARTS * sizeof(float);
    if (!e->amax_dev) HIP_TRY(hipMalloc((void**)&e->amax_dev, bytes));
    if (!e->amax_host) HIP_TRY(hipHostMalloc((void**)&e->amax_host, bytes));
    return APZ_OK;
}

// The largest |a| the layer's weights allow: 2^-a goes into 1 / S[co] = 2^-k of the bias FMA, and 2^-(a + k) must be a
// normal float for every output channel (the subnormal case is exact only while fp32 denormals are enabled: see the DGRAD
// comment in trunk15_wino3h16.h).  Reads the layer's 1 / S from the device: the packing kernels compute them there.
// Synchronous.
int clamp_act_exponent(apz_engine* e, const ConvLayer& L, int a, int* out) {
    a = std::max(-apz::ACT_EXP_MAX, std::min(apz::ACT_EXP_MAX, a));
    if (a != 0 && L.bias3h) {
        float inv_s[128];
        HIP_TRY(hipMemcpyAsync(inv_s, L.bias3h + 128, sizeof(inv_s), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        int kmin = 1000, kmax = -1000;
        for (float v : inv_s) {
            int ex;
            std::frexp((double)v, &ex);               // 1 / S = 2^-k = 0.5 x 2^(1 - k)
            kmin = std::min(kmin, 1 - ex);
            kmax = std::max(kmax, 1 - ex);
        }
        a = std::max(-126 - kmin, std::min(126 - kmax, a));   // -126 <= a + k <= 126 for every channel
    }
    *out = a;
    return APZ_OK;
}

// after the stream synchronisation behind a measuring forward: the maxima of the `count` trunk inputs
void fold_act_maxima(apz_engine* e, int n, int count, float* m) {
    const int parts = apz::ActMax::grid_for((long)n * 128 * (apz::Trunk15::GPLANE / 4));
    for (int l = 0; l < count; l++) {
        float v = 0.f;
        for (int i = 0; i < parts; i++) v = std::fmax(v, e->amax_host[(size_t)l * apz::ActMax::MAX_PARTS + i]);
        m[l] = v;
    }
}

// apz_set_act_scale_auto: behind the exact repeat of an overflowed forward of n boards (stream drained).  Only ever lowers
// an exponent; a non-finite maximum (the exact forward overflowed too) leaves all of them alone.
int lower_act_exponents(apz_engine* e, int n) {
    const int count = (int)e->convs.size() - 1;
    std::vector<float> m(count);
    fold_act_maxima(e, n, count, m.data());
    for (float v : m)
        if (!std::isfinite(v)) return APZ_OK;
    bool changed = false;
    for (int l = 0; l < count; l++) {
        ConvLayer& L = e->convs[l + 1];
        int a = std::min(L.act_exp, apz::act_exponent_for(m[l]));
        if (int rc = clamp_act_exponent(e, L, a, &a)) return rc;
        if (a < L.act_exp) {
            L.act_exp = a;
            changed = true;
        }
    }
    if (changed) drop_forward_graphs(e);          // a captured launch sequence holds the old exponents
    return APZ_OK;
}

// The exact-fp32 repeat of an overflowed forward of n boards; with apz_set_act_scale_auto on it measures the trunk inputs
// on the way and lowers the exponents behind it.  Returns with the stream drained.  `run(mode)` queues the forward.
template <class F>
int repeat_exact(apz_engine* e, int n, F run) {
    FwdMode m;
    m.exact = true;
    m.measure_max = e->act_auto && e->amax_dev && n > 0;
    int rc = run(m);
    e->ovf_repeats++;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    // (the boards the repeat's own forward ran: n, or 8 n under APZ_SYM_MEAN8 -- forward_dev left them in last_n)
    return m.measure_max ? lower_act_exponents(e, e->last_n) : APZ_OK;
}

// one measuring forward of n boards on the exact-fp32 kernels (`run(mode)` stages and queues it), then the exponents from
// the maxima
template <class F>
int calibrate_trunk(apz_engine* e, int n, float* layer_max_out, int count, F run) {
    if (int rc = act_scale_supported(e)) return rc;
    if (!e->loaded) return fail(APZ_E_STATE, "weights not loaded");
    const int layers = (int)e->convs.size() - 1;
    if (count != layers) return fail(APZ_E_ARG, "calibration: count must be 2 * n_blocks = " + std::to_string(layers));
    if (n < 1 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "calibration: batch must be in [1, max_batch]");
    if (count == 0) return APZ_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (int rc = act_scale_buffers(e)) return rc;
    FwdMode measuring;                            // (no overflow word armed: nothing here counts as an overflow)
    measuring.exact = measuring.measure_max = true;
    if (int rc = run(measuring)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    resolve_pending(e);
    std::vector<float> m(count);
    fold_act_maxima(e, n, count, m.data());
    if (layer_max_out) std::memcpy(layer_max_out, m.data(), count * sizeof(float));
    for (int l = 0; l < count; l++)
        if (!std::isfinite(m[l]))
            return fail(APZ_E_STATE, "calibration: the input of trunk convolution " + std::to_string(l) +
                                         " is not finite in exact fp32; the exponents are unchanged");
    std::vector<int> eff(count);
    for (int l = 0; l < count; l++)
        if (int rc2 = clamp_act_exponent(e, e->convs[l + 1], apz::act_exponent_for(m[l]), &eff[l])) return rc2;
    drop_forward_graphs(e);
    std::vector<int> old(count);
    for (int l = 0; l < count; l++) {
        old[l] = e->convs[l + 1].act_exp;
        e->convs[l + 1].act_exp = eff[l];
    }
    // The maxima are taken behind the ReLU, which turns a NaN into 0: a layer whose exact-fp32 sums are inf - inf shows a
    // maximum of 0, not a non-finite one.  So the new exponents prove themselves on their own batch: the same forward on
    // the f16x2 kernel (whatever the batch size), whose non-finite check sits in front of the ReLU, must not raise the word.
    FwdMode proving = armed(e, APZ_MAX_SLOTS);
    proving.batched = true;
    e->ovf_host[APZ_MAX_SLOTS] = 0;
    const int rc = run(proving);
    hipError_t he = hipStreamSynchronize(e->stream);
    resolve_pending(e);
    const bool raised = e->ovf_host[APZ_MAX_SLOTS] != 0;
    e->ovf_host[APZ_MAX_SLOTS] = 0;
    if (rc || he != hipSuccess || raised) {
        for (int l = 0; l < count; l++) e->convs[l + 1].act_exp = old[l];
        if (rc) return rc;
        if (he != hipSuccess) return fail(APZ_E_HIP, std::string("calibration: ") + hipGetErrorString(he));
        return fail(APZ_E_STATE, "calibration: the batch is not finite on the f16x2 kernel with its own exponents (a layer "
                                 "overflows in exact fp32 too); the exponents are unchanged");
    }
    return APZ_OK;
}

// The forward of the synchronous entry points: `run(mode)` queues it with the synchronous overflow word armed.
// APZ_ARITH_F16X2: collected here -- wait for the stream, look at the word and, if an activation left the fp16 range, run
// the same forward again on the exact-fp32 trunk kernel.  Other arithmetics: queued, nothing more.
template <class F>
int forward_guarded(apz_engine* e, int n, F run) {
    const FwdMode m = armed(e, APZ_MAX_SLOTS);
    if (!m.ovf) return run(m);
    unsigned& word = e->ovf_host[APZ_MAX_SLOTS];
    word = 0;
    if (int rc = run(m)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (word) {
        word = 0;
        return repeat_exact(e, n, run);
    }
    return APZ_OK;
}

// ... of n boards into e->probs / e->values, and those to the caller
template <class F>
int forward_to_host(apz_engine* e, int n, F run, float* probs_host, float* values_host) {
    if (int rc = forward_guarded(e, n, run)) return rc;
    return collect_to_host(e, n, probs_host, values_host);
}

// dihedral index tables (train_mxnet.py:115-135) on square boards
void build_perms(int N, std::vector<int>& ps, std::vector<int>& pp) {
    typedef std::vector<int> Grid;
    auto rot90 = [N](const Grid& a) { Grid r(N * N); for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) r[i * N + j] = a[j * N + (N - 1 - i)]; return r; };
    auto fliplr = [N](const Grid& a) { Grid r(N * N); for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) r[i * N + j] = a[i * N + (N - 1 - j)]; return r; };
    auto flipud = [N](const Grid& a) { Grid r(N * N); for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) r[i * N + j] = a[(N - 1 - i) * N + j]; return r; };
    Grid id(N * N);
    for (int i = 0; i < N * N; i++) id[i] = i;
    ps.clear();
    pp.clear();
    Grid s = id, p = flipud(id);
    for (int k = 1; k <= 4; k++) {
        s = rot90(s);
        p = rot90(p);
        Grid po = flipud(p);
        ps.insert(ps.end(), s.begin(), s.end());
        pp.insert(pp.end(), po.begin(), po.end());
        Grid sf = fliplr(s), pf = flipud(fliplr(p));
        ps.insert(ps.end(), sf.begin(), sf.end());
        pp.insert(pp.end(), pf.begin(), pf.end());
    }
}

// ---- weights: apz_load_weights and apz_load_weights_dev share everything below

typedef std::map<std::string, const float*> ParamPtrs;

// name -> pointer of the caller's table (host or device pointers alike); every parameter of the net must be there, at its size
int check_param_table(apz_engine* e, const char* const* names, const void* const* ptrs, const int64_t* sizes, int n, ParamPtrs& P) {
    std::map<std::string, int64_t> S;
    for (int i = 0; i < n; i++) {
        P[names[i]] = (const float*)ptrs[i];
        S[names[i]] = sizes[i];
    }
    for (auto& p : e->params) {
        auto it = S.find(p.name);
        if (it == S.end()) return fail(APZ_E_ARG, "missing parameter " + p.name);
        if (it->second != p.size)
            return fail(APZ_E_ARG, "parameter " + p.name + " has " + std::to_string(it->second) + " elements, expected " +
                                       std::to_string(p.size));
    }
    return APZ_OK;
}

// Zeroed on the engine's stream, in front of the first packing kernels: those write the value slots of a layout only, and
// the forward kernels load the pad slots next to them with 16-byte reads.  Keeps a buffer it finds (a first load that failed
// half way is repeated).
template <typename T>
int alloc_zeroed(apz_engine* e, T** dst, size_t bytes) {
    if (*dst) return APZ_OK;
    HIP_TRY(hipMalloc((void**)dst, bytes));
    HIP_TRY(hipMemsetAsync(*dst, 0, bytes, e->stream));
    return APZ_OK;
}

// Every weight buffer the engine's configuration needs (net, ring, small8, frame_s through ring, trunk_arith -- fixed from
// the first load on: apz_set_trunk_arith), sized by the layouts' own constants, plus the fold scratch and the staging
// buffer of apz_load_weights.  The first apz_load_weights calls it; nothing else allocates a weight buffer.
int alloc_packed(apz_engine* e) {
    int rc = APZ_OK;
    auto get = [&](auto** dst, size_t bytes) {
        if (rc == APZ_OK) rc = alloc_zeroed(e, dst, bytes);
    };
    const bool f16x2 = e->trunk_arith == APZ_ARITH_F16X2;
    static_assert(apz::Wino3H16::UPK_BYTES == apz::Wino3H::UPK_BYTES, "both f16x2 kernels share the layer's upk3h buffer");
    for (auto& L : e->convs) {
        const bool wino = e->ring && &L != &e->convs[0];     // a 128 -> 128 layer of the 15x15 trunk kernels
        const size_t frags = (size_t)(L.cout / 16) * (L.cin_pad / 4) * 64;
        get(&L.wpk, frags * (wino ? 12 : 9) * sizeof(float));
        get(&L.bias, L.cout * sizeof(float));
        if (e->small8) get(&L.wpk12, frags * 12 * sizeof(float));
        // (generic engines take APZ_ARITH_F16X2 on 15x15 boards only: apz_set_trunk_arith)
        if ((e->small8 || !e->ring) && f16x2 && apz::Conv8H::supports(L.cin, L.cout)) {
            get(&L.wpk8h, apz::Conv8H::pk_bytes(L.cin, L.cout));
            get(&L.bias8h, 2 * (size_t)L.cout * sizeof(float));
        }
        if (wino) {
            get(&L.upk2, apz::WinoPack::UPK_FLOATS * sizeof(float));
            get(&L.upk3s, apz::WinoPackSmall::UPK_FLOATS * sizeof(float));
        }
        if (wino && e->trunk_arith == APZ_ARITH_BF16X3) get(&L.upk3b, apz::Wino3B::UPK_BYTES);
        if (wino && f16x2) {
            get(&L.upk3h, apz::Wino3H::UPK_BYTES);
            get(&L.bias3h, apz::Wino3H::BIAS_FLOATS * sizeof(float));
        }
    }
    const size_t C = e->clast, hw = e->hw;
    get(&e->w6, 6 * C * sizeof(float));
    get(&e->b6, 6 * sizeof(float));
    get(&e->wfc_pk, ((hw + 15) / 16) * ((hw + 7) / 8) * 64 * 8 * sizeof(float));
    get(&e->bfc, hw * sizeof(float));
    get(&e->wv, 2 * hw * sizeof(float));
    get(&e->bv, sizeof(float));
    if (e->small8) get(&e->wfc_raw, hw * 4 * hw * sizeof(float));
    get(&e->fold_ws, 2 * (size_t)e->cmax * sizeof(double));
    size_t floats = 0;
    for (auto& p : e->params) floats += (size_t)p.size;
    get(&e->stage, floats * sizeof(float));
    return rc;
}

// Raw parameters (DEVICE pointers) -> every packed buffer of the engine, queued on `st`: per layer the BatchNorm fold, then
// one packer per form the layer has; the heads (two 1x1 conv_act, fix_gamma default, folded into one [6][C] matrix) and the
// FullyConnected layers last.  fold_ws is reused from layer to layer: the stream orders its users.
int pack_all(apz_engine* e, const ParamPtrs& P, hipStream_t st) {
    double* scale = e->fold_ws;
    double* shift = e->fold_ws + e->cmax;
    auto fold = [&](const std::string& conv, const std::string& bn, const std::string& mean_sfx, const std::string& var_sfx,
                    bool fix_gamma, int cout, float* bias_out) {
        hipLaunchKernelGGL(apz::fold_bn_kernel, dim3((cout + 63) / 64), dim3(64), 0, st, P.at(conv + "_bias"),
                           fix_gamma ? (const float*)nullptr : P.at(bn + "_gamma"), P.at(bn + "_beta"), P.at(bn + mean_sfx),
                           P.at(bn + var_sfx), scale, shift, bias_out, cout, (double)BN_EPS);
    };
    for (auto& L : e->convs) {
        fold(L.name, L.bn, L.mean_sfx, L.var_sfx, L.fix_gamma, L.cout, L.bias);
        const float* w = P.at(L.name + "_weight");   // [cout][cin][3][3]
        const int n4 = L.cin_pad / 4, ncot = L.cout / 16;
        const int total = ncot * n4 * 9 * 64;
        const dim3 direct_grid(std::min((total + 255) / 256, 2048));
        hipLaunchKernelGGL(apz::pack_direct_kernel, direct_grid, dim3(256), 0, st, w, scale, L.wpk, L.cin, n4, ncot,
                           (int)(L.upk2 != nullptr));
        if (L.upk2)
            hipLaunchKernelGGL(apz::pack_wino_folded_kernel, dim3(128 * 128 / 256), dim3(256), 0, st, w, scale, L.upk2, L.upk3s);
        if (L.upk3b)
            hipLaunchKernelGGL(apz::pack_wino3b_folded_kernel, dim3(128 * 128 / 256), dim3(256), 0, st, w, scale,
                               (unsigned short*)L.upk3b);
        if (L.upk3h) {
            if (e->f16x2_k8)
                hipLaunchKernelGGL(apz::pack_wino3h_folded_kernel<apz::Wino3H>, dim3(128), dim3(128), 0, st, w, scale, shift,
                                   (unsigned short*)L.upk3h, L.bias3h);
            else
                hipLaunchKernelGGL(apz::pack_wino3h_folded_kernel<apz::Wino3H16>, dim3(128), dim3(128), 0, st, w, scale, shift,
                                   (unsigned short*)L.upk3h, L.bias3h);
        }
        if (L.wpk12)
            hipLaunchKernelGGL(apz::pack_direct_kernel, direct_grid, dim3(256), 0, st, w, scale, L.wpk12, L.cin, n4, ncot, 1);
        if (L.wpk8h)
            hipLaunchKernelGGL(apz::pack_conv8h_kernel, dim3(L.cout), dim3(256), 0, st, w, scale, shift, (unsigned short*)L.wpk8h,
                               L.bias8h, L.cin, L.cout);
        HIP_TRY(hipGetLastError());
    }
    const int C = e->clast, hw = e->hw;
    fold("conv3_1_1", "conv3_1_1", "_mean", "_var", true, 4, nullptr);
    hipLaunchKernelGGL(apz::pack_head_conv_kernel, dim3((4 * C + 255) / 256), dim3(256), 0, st, P.at("conv3_1_1_weight"), scale,
                       shift, e->w6, e->b6, 4, 0, C);
    fold("conv3_2_1", "conv3_2_1", "_mean", "_var", true, 2, nullptr);
    hipLaunchKernelGGL(apz::pack_head_conv_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, st, P.at("conv3_2_1_weight"), scale,
                       shift, e->w6, e->b6, 2, 4, C);
    const int ntile = (hw + 15) / 16, KG = (hw + 7) / 8;
    hipLaunchKernelGGL(apz::pack_fc_kernel, dim3(std::min((ntile * KG * 512 + 255) / 256, 2048)), dim3(256), 0, st,
                       P.at("fc_3_1_1_weight"), e->wfc_pk, hw, ntile, KG);
    HIP_TRY(hipGetLastError());
    if (e->wfc_raw)     // head8_kernel reads the policy FullyConnected weight as stored
        HIP_TRY(hipMemcpyAsync(e->wfc_raw, P.at("fc_3_1_1_weight"), (size_t)hw * 4 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->bfc, P.at("fc_3_1_1_bias"), hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->wv, P.at("fc_3_2_1_weight"), 2 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->bv, P.at("fc_3_2_1_bias"), sizeof(float), hipMemcpyDeviceToDevice, st));
    return APZ_OK;
}

}  // namespace

namespace {
struct StreamScope {      // run the engine's launch helpers on a caller-supplied stream
    apz_engine* e;
    hipStream_t saved;
    StreamScope(apz_engine* e_, void* s) : e(e_), saved(e_->stream) {
        if (s != APZ_ENGINE_STREAM) e->stream = (hipStream_t)s;   // NULL is a valid handle: the null stream
        // The training entry points share per-engine scratch (the DeviceBuffers of apz_engine: bn_part, wgw_scratch,
        // head_scratch, adam_tab, guard_part, gather_entries, wino_scratch, conv15h_scratch, conv15h_tab; and fold_ws).  Calls on ONE stream are ordered by the
        // stream; a caller that switches streams gets the new stream ordered behind everything queued on the previous
        // one, so two streams never work on the scratch at once.
        if (e->scratch_stream_valid && e->scratch_stream != e->stream) (void)stream_wait(e, e->stream, e->scratch_stream);
        e->scratch_stream = e->stream;
        e->scratch_stream_valid = true;
    }
    ~StreamScope() { e->stream = saved; }
};

// The scope of a training entry point: the engine's lock, its device made current, `stream` in place of the engine's own
// -- in that order (StreamScope records events on the current device, and it is what keeps two streams off the shared
// scratch) -- then `body() -> int`, and after a body that succeeded the verdict of hipGetLastError.
template <class F>
int train_call(apz_engine* e, void* stream, F body) {
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    StreamScope sc(e, stream);
    if (int rc = body()) return rc;
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

// A runtime flag as a template argument: f(std::true_type{}) or f(std::false_type{}), each kernel and launch written once
template <class F>
auto with_flag(bool flag, F f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}
template <int V>
using int_c = std::integral_constant<int, V>;
}  // namespace

extern "C" {

const char* apz_last_error(void) { return g_err.c_str(); }
int apz_version(void) { return 1; }

int apz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void apz_destroy(apz_engine* e) {
    if (!e) return;
    hipSetDevice(e->cfg.device);
    if (e->stream) hipStreamSynchronize(e->stream);
    resolve_pending(e);
    drop_forward_graphs(e);
    for (auto ev : e->free_events) hipEventDestroy(ev);
    for (auto& l : e->convs) {
        if (l.wpk) hipFree(l.wpk);
        if (l.upk2) hipFree(l.upk2);
        if (l.upk3s) hipFree(l.upk3s);
        if (l.upk3b) hipFree(l.upk3b);
        if (l.upk3h) hipFree(l.upk3h);
        if (l.bias3h) hipFree(l.bias3h);
        if (l.wpk8h) hipFree(l.wpk8h);
        if (l.bias8h) hipFree(l.bias8h);
        if (l.wpk12) hipFree(l.wpk12);
        if (l.bias) hipFree(l.bias);
    }
    void* dev[] = {e->w6, e->b6, e->wfc_pk, e->bfc, e->wv, e->bv, e->act[0], e->act[1], e->act[2], e->planes,
                   e->featp, e->featv, e->probs, e->values, e->codes, e->perm_s, e->perm_p, e->smp_vis, e->smp_pi, e->smp_mv, e->zeros256,
                   e->fc_logits, e->fold_ws, e->stage, e->wfc_raw, e->amax_dev, e->fplanes};
    for (void* p : dev)
        if (p) hipFree(p);
    for (DeviceBuffer* b : {&e->bn_part, &e->wgw_scratch, &e->head_scratch, &e->adam_tab, &e->guard_part, &e->gather_entries,
                            &e->wino_scratch[0], &e->wino_scratch[1], &e->conv15h_scratch, &e->conv15h_tab})
        b->release();
    if (e->perm_pinv) hipFree(e->perm_pinv);
    if (e->occ) hipFree(e->occ);
    for (auto& st : e->sym) {
        void* stage[] = {st.codes, st.k, st.probs, st.values};
        for (void* p : stage)
            if (p) hipFree(p);
    }
    e->w3s.release();
    e->w3hs.release();
    if (e->ovf_host) hipHostFree(e->ovf_host);
    if (e->amax_host) hipHostFree(e->amax_host);
    for (auto& sl : e->slots) {
        if (sl.h_codes) hipHostFree(sl.h_codes);
        if (sl.h_probs) hipHostFree(sl.h_probs);
        if (sl.h_values) hipHostFree(sl.h_values);
        if (sl.done) hipEventDestroy(sl.done);
    }
    void* host[] = {e->h_planes, e->h_probs, e->h_values, e->h_codes};
    for (void* p : host)
        if (p) hipHostFree(p);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

apz_engine* apz_create(const apz_config* cfg) {
    if (!cfg || cfg->height < 1 || cfg->width < 1 || cfg->max_batch < 1 || (cfg->c_in != 9 && cfg->c_in != 4)) {
        fail(APZ_E_ARG, "bad config (c_in must be 9 or 4)");
        return nullptr;
    }
    if (cfg->height != cfg->width || cfg->height < 6 || cfg->height > 15) {
        fail(APZ_E_UNSUPPORTED, "boards are square, 6x6 to 15x15 (not 10x10): 15x15 and 8x8 have kernels of their own, the other sizes run "
                                "the 128-filter residual net on the 15x15 trunk kernels (csrc/frame15.h)");
        return nullptr;
    }
    const bool framed = apz::Frame15::framed_side(cfg->height);
    if (cfg->height == 10) {
        fail(APZ_E_UNSUPPORTED, "10x10 boards are not supported: 15x15 and 8x8 have kernels of their own, 6x6, 7x7, 9x9 and 11x11 "
                                "to 14x14 run the 128-filter residual net on the 15x15 trunk kernels (csrc/frame15.h)");
        return nullptr;
    }
    if (framed && (cfg->net_kind != APZ_NET_RESNET || cfg->n_filter != 128)) {
        fail(APZ_E_UNSUPPORTED, "boards of 6x6 to 14x14 other than 8x8 and 10x10 run the residual net with 128 filters only (the simple "
                                "net and 64 / 256 filters exist at 15x15 and 8x8)");
        return nullptr;
    }
    if (cfg->net_kind == APZ_NET_RESNET &&
        ((cfg->n_filter != 64 && cfg->n_filter != 128 && cfg->n_filter != 256) || cfg->n_blocks < 0)) {
        fail(APZ_E_UNSUPPORTED, "n_filter must be 64, 128 or 256");
        return nullptr;
    }
    if (cfg->net_kind != APZ_NET_RESNET && cfg->net_kind != APZ_NET_SIMPLE) {
        fail(APZ_E_ARG, "unknown net_kind");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        fail(APZ_E_HIP, "no HIP device: libalphapig_hip needs an AMD GPU (there is no CPU fallback)");
        return nullptr;
    }
    if (cfg->device < 0 || cfg->device >= ndev) {
        fail(APZ_E_ARG, "device ordinal out of range");
        return nullptr;
    }
    apz_engine* e = new apz_engine();
    e->cfg = *cfg;
    e->hw = cfg->height * cfg->width;
    e->code_stride = (e->hw + 1 + 15) / 16 * 16;
    build_tables(e);
    auto bail = [&](const char* what, hipError_t err) -> apz_engine* {
        fail(APZ_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
        apz_destroy(e);
        return nullptr;
    };
    hipError_t err;
    if ((err = hipSetDevice(cfg->device)) != hipSuccess) return bail("hipSetDevice", err);
    hipDeviceProp_t prop;
    if ((err = hipGetDeviceProperties(&prop, cfg->device)) != hipSuccess) return bail("hipGetDeviceProperties", err);
    e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        const char* k8 = getenv("APZ_F16X2_K8");
        e->f16x2_k8 = k8 && atoi(k8) != 0;
    }
    if ((err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess)
        return bail("hipStreamCreate", err);
    e->frame_s = framed ? cfg->height : 0;
    e->ring = cfg->net_kind == APZ_NET_RESNET && cfg->n_filter == 128 && (framed || (cfg->height == 15 && cfg->width == 15));
    e->small8 = cfg->height == 8 && cfg->width == 8;
    e->act_ps = e->ring ? apz::Trunk15::GPLANE : e->hw;
    e->act_rs = e->ring ? apz::Trunk15::GROW : cfg->width;
    const size_t B = cfg->max_batch, hw = e->hw;
    const size_t act_bytes = B * e->cmax * (size_t)e->act_ps * sizeof(float);
    for (int i = 0; i < 3; i++)
    {
        if ((err = hipMalloc((void**)&e->act[i], act_bytes)) != hipSuccess) return bail("hipMalloc(act)", err);
        // rows16 pad columns must read as zero; they are never written with anything else
        if ((err = hipMemset(e->act[i], 0, act_bytes)) != hipSuccess) return bail("hipMemset(act)", err);
    }
    if ((err = hipMalloc((void**)&e->planes, B * 9 * hw * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if (framed && (err = hipMalloc((void**)&e->fplanes, B * 9 * apz::Frame15::CELLS * sizeof(float))) != hipSuccess)
        return bail("hipMalloc(framed planes)", err);
    if ((err = hipMalloc((void**)&e->featp, B * 4 * hw * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc((void**)&e->featv, B * 2 * hw * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc((void**)&e->probs, B * hw * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc((void**)&e->fc_logits, B * ((hw + 15) / 16 * 16) * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc((void**)&e->values, B * sizeof(float))) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMalloc((void**)&e->codes, B * e->code_stride)) != hipSuccess) return bail("hipMalloc", err);
    if ((err = hipMemset(e->codes, 0, B * e->code_stride)) != hipSuccess) return bail("hipMemset(codes)", err);   // empty boards: apz_prewarm's input
    if ((err = hipHostMalloc((void**)&e->h_planes, B * 9 * hw * sizeof(float))) != hipSuccess) return bail("hipHostMalloc", err);
    if ((err = hipHostMalloc((void**)&e->h_probs, B * hw * sizeof(float))) != hipSuccess) return bail("hipHostMalloc", err);
    if ((err = hipHostMalloc((void**)&e->h_values, B * sizeof(float))) != hipSuccess) return bail("hipHostMalloc", err);
    if ((err = hipHostMalloc((void**)&e->h_codes, B * e->code_stride)) != hipSuccess) return bail("hipHostMalloc", err);
    if (cfg->height == cfg->width) {
        std::vector<int> ps, pp;
        build_perms(cfg->height, ps, pp);
        if (upload(&e->perm_s, ps) || upload(&e->perm_p, pp)) {
            apz_destroy(e);
            return nullptr;
        }
    }
    return e;
}

int apz_param_count(apz_engine* e) { return e ? (int)e->params.size() : fail(APZ_E_ARG, "null engine"); }

const char* apz_param_name(apz_engine* e, int i) {
    if (!e || i < 0 || i >= (int)e->params.size()) return nullptr;
    return e->params[i].name.c_str();
}

int64_t apz_param_size(apz_engine* e, int i) {
    if (!e || i < 0 || i >= (int)e->params.size()) return -1;
    return e->params[i].size;
}

int apz_load_weights(apz_engine* e, const char* const* names, const float* const* ptrs, const int64_t* sizes, int n) {
    if (!e || !names || !ptrs || !sizes) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    ParamPtrs host, dev;
    if (int rc = check_param_table(e, names, (const void* const*)ptrs, sizes, n, host)) return rc;
    // drained: no forward reads the weights any more, and a device-side refresh on another stream (which the engine's
    // stream was ordered behind) is through with fold_ws
    HIP_TRY(hipStreamSynchronize(e->stream));
    drop_forward_graphs(e);
    if (!e->loaded)
        if (int rc = alloc_packed(e)) return rc;
    // the host tensors go to the staging buffer (allocated once: no hipMalloc / hipFree per load, which would stall every
    // engine on the device), and from there through the kernels every refresh runs
    size_t off = 0;
    for (auto& p : e->params) {
        HIP_TRY(hipMemcpyAsync(e->stage + off, host.at(p.name), (size_t)p.size * sizeof(float), hipMemcpyHostToDevice, e->stream));
        dev[p.name] = e->stage + off;
        off += (size_t)p.size;
    }
    if (int rc = pack_all(e, dev, e->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->loaded = true;
    // the activation exponents are engine state and survive the load; the new 1 / S may only narrow their range
    for (auto& L : e->convs)
        if (L.act_exp != 0)
            if (int rc = clamp_act_exponent(e, L, L.act_exp, &L.act_exp)) return rc;
    return APZ_OK;
}

int apz_forward(apz_engine* e, const void* planes_dev, int n, void* probs_dev, void* values_dev, void* logits_dev,
                void* vlogits_dev) {
    if (!e || !planes_dev || !probs_dev || !values_dev) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    // (APZ_ARITH_F16X2: returns with the stream drained -- the overflow word has to be read before the results are used)
    return forward_guarded(e, n, [&](const FwdMode& m) {
        return forward_dev(e, m, (const float*)planes_dev, nullptr, n, (float*)probs_dev, (float*)values_dev, (float*)logits_dev,
                           (float*)vlogits_dev);
    });
}

int apz_forward_host(apz_engine* e, const float* planes_host, int n, float* probs_host, float* values_host) {
    if (!e || !planes_host || !probs_host || !values_host) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (n == 0) return APZ_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (int rc = stage_planes(e, planes_host, n)) return rc;
    return forward_to_host(e, n, [&](const FwdMode& m) { return forward_dev(e, m, e->planes, nullptr, n, e->probs, e->values); },
                           probs_host, values_host);
}

int apz_forward_codes_async(apz_engine* e, const uint8_t* codes_pinned, int n, float* probs_pinned,
                            float* values_pinned) {
    if (!e || !codes_pinned || !probs_pinned || !values_pinned) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (e->cfg.c_in != 9 && e->cfg.c_in != 4) return fail(APZ_E_STATE, "bad c_in");
    if (n == 0) return APZ_OK;
    if (int rc = sym_batch_ok(e, n)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t hw = e->hw;
    HIP_TRY(hipMemcpyAsync(e->codes, codes_pinned, (size_t)n * e->code_stride, hipMemcpyHostToDevice, e->stream));
    // (APZ_ARITH_F16X2: the forward is collected here, see forward_guarded -- the copies below are queued behind it)
    int rc = forward_guarded(e, n, [&](const FwdMode& m) { return forward_codes_sym(e, m, APZ_MAX_SLOTS, e->codes, n, e->probs, e->values); });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(probs_pinned, e->probs, n * hw * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(values_pinned, e->values, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    return APZ_OK;
}

int apz_forward_codes_host(apz_engine* e, const uint8_t* codes_host, int n, float* probs_host, float* values_host) {
    if (!e || !codes_host || !probs_host || !values_host) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (n == 0) return APZ_OK;
    if (int rc = sym_batch_ok(e, n)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (int rc = stage_codes(e, codes_host, n)) return rc;
    return forward_to_host(e, n, [&](const FwdMode& m) { return forward_codes_sym(e, m, APZ_MAX_SLOTS, e->codes, n, e->probs, e->values); },
                           probs_host, values_host);
}

// batches above this are a handful of long kernels: nothing to gain from a graph
constexpr int FWD_GRAPH_MAX_BOARDS = 64;

int apz_submit_codes(apz_engine* e, int slot, const uint8_t* codes_host, int n) {
    if (!e || !codes_host) return fail(APZ_E_ARG, "null argument");
    if (slot < 0 || slot >= APZ_MAX_SLOTS) return fail(APZ_E_ARG, "slot out of range");
    if (n < 1 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch must be in [1, max_batch]");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    apz_engine::Slot& sl = e->slots[slot];
    if (sl.busy) return fail(APZ_E_STATE, "slot still in flight: call apz_wait first");
    if (int rc = sym_batch_ok(e, n)) return rc;
    const size_t B = e->cfg.max_batch, hw = e->hw;
    if (!sl.h_codes) {
        // Zero-copy slots: the 240-B/leaf codes and the 904-B/leaf results live in pinned,
        // device-mapped host memory.  The encoder reads the codes and the head kernel writes
        // probs/values straight over PCIe -- no blit kernels (and their ~25 us launch gaps)
        // around the forward.
        HIP_TRY(hipHostMalloc((void**)&sl.h_codes, B * e->code_stride, hipHostMallocMapped));
        HIP_TRY(hipHostMalloc((void**)&sl.h_probs, B * hw * sizeof(float), hipHostMallocMapped));
        HIP_TRY(hipHostMalloc((void**)&sl.h_values, B * sizeof(float), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&sl.d_codes, sl.h_codes, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&sl.d_probs, sl.h_probs, 0));
        HIP_TRY(hipHostGetDevicePointer((void**)&sl.d_values, sl.h_values, 0));
        HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    std::memcpy(sl.h_codes, codes_host, (size_t)n * e->code_stride);
    // (the codes are read straight from the pinned slot)
    const FwdMode m = armed(e, slot);                         // the slot's overflow word: read by apz_wait
    if (m.ovf) e->ovf_host[slot] = 0;
    auto launch_all = [&]() { return forward_codes_sym(e, m, slot, sl.d_codes, n, sl.d_probs, sl.d_values); };
    int rc = APZ_OK;
    const long key = ((long)slot << 32) | (long)n;
    const bool graphable = e->use_graphs && !e->profiling && n <= FWD_GRAPH_MAX_BOARDS && e->loaded;
    auto it = graphable ? e->fwd_graphs.find(key) : e->fwd_graphs.end();
    if (it != e->fwd_graphs.end()) {
        HIP_TRY(hipGraphLaunch(it->second, e->stream));
        e->last_n = e->sym_mode == APZ_SYM_MEAN8 ? 8 * n : n;
    } else if (graphable && ++e->fwd_seen[key] >= 3 && !e->w3s.near_wrap() && !e->w3hs.near_wrap()) {
        // (third use: every lazy allocation / attribute / ticket reset of this shape has happened outside the capture --
        // need_lds is per kernel, and the two plain submissions before this one launched the kernels the capture launches:
        // a submission's mode is armed(e, slot) every time, so its kernels follow from what trunk_route and first_layer read
        // of the engine (weights, arithmetic, exponents, uniform, the test selection), and every setter of that goes through
        // drop_forward_graphs, which starts the count again)
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
        rc = launch_all();
        const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
        if (rc) {
            if (graph) hipGraphDestroy(graph);
            return rc;
        }
        if (ce != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            if (graph) hipGraphDestroy(graph);
            (void)hipGetLastError();
            e->use_graphs = false;          // this runtime cannot capture the sequence: plain launches from here on
            rc = launch_all();
            if (rc) return rc;
        } else {
            hipGraphDestroy(graph);
            e->fwd_graphs[key] = exec;
            HIP_TRY(hipGraphLaunch(exec, e->stream));
        }
    } else {
        rc = launch_all();
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(sl.done, e->stream));
    sl.n = n;
    sl.busy = true;
    return APZ_OK;
}

int apz_wait(apz_engine* e, int slot, float* probs_host, float* values_host) {
    if (!e || !probs_host || !values_host) return fail(APZ_E_ARG, "null argument");
    // (no engine lock: a slot is owned by the one thread that submitted into it, and holding the lock across the
    // event wait would stop the other pipeline groups from submitting behind this batch)
    if (slot < 0 || slot >= APZ_MAX_SLOTS) return fail(APZ_E_ARG, "slot out of range");
    apz_engine::Slot& sl = e->slots[slot];
    if (!sl.busy) return fail(APZ_E_STATE, "nothing submitted in this slot");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipEventSynchronize(sl.done));
    if (e->ovf_host && e->ovf_host[slot]) {
        // an activation of this batch left the fp16 range (trunk15_wino3h.h): the same batch again on the exact-fp32 kernel
        EngineLock guard(e->submit_lock);
        e->ovf_host[slot] = 0;
        int rc = repeat_exact(e, sl.n, [&](const FwdMode& m) { return forward_codes_sym(e, m, slot, sl.d_codes, sl.n, sl.d_probs, sl.d_values); });
        if (rc) return rc;
    }
    std::memcpy(probs_host, sl.h_probs, (size_t)sl.n * e->hw * sizeof(float));
    std::memcpy(values_host, sl.h_values, (size_t)sl.n * sizeof(float));
    sl.busy = false;
    return sl.n;
}

void* apz_host_alloc(int64_t bytes) {
    void* p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes) != hipSuccess) {
        fail(APZ_E_HIP, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

void apz_host_free(void* p) {
    if (p) hipHostFree(p);
}

int apz_encode_planes(apz_engine* e, const void* codes_dev, int n, int n_planes, void* planes_dev) {
    if (!e || !codes_dev || !planes_dev) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (n_planes != 9 && n_planes != 4) return fail(APZ_E_ARG, "n_planes must be 9 or 4");
    if (n <= 0) return APZ_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    Timed tm(e, APZ_K_ENCODE);
    const int total = n * e->hw;
    hipLaunchKernelGGL(apz::encode_planes_kernel, dim3(std::min((total + 255) / 256, e->num_cu * 8)), dim3(256), 0,
                       e->stream, (const unsigned char*)codes_dev, (float*)planes_dev, n, e->cfg.height, e->cfg.width,
                       e->code_stride, n_planes);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

int apz_augment8(apz_engine* e, const void* planes_dev, const void* pi_dev, int n, int c, void* planes_out_dev,
                 void* pi_out_dev) {
    if (!e || !planes_dev || !pi_dev || !planes_out_dev || !pi_out_dev) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (!e->perm_s) return fail(APZ_E_UNSUPPORTED, "augmentation needs a square board");
    if (n <= 0) return APZ_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    const long total = (long)n * 8 * (c + 1) * e->hw;
    hipLaunchKernelGGL(apz::augment8_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 16)), dim3(256),
                       0, e->stream, (const float*)planes_dev, (const float*)pi_dev, e->perm_s, e->perm_p,
                       (float*)planes_out_dev, (float*)pi_out_dev, n, c, e->hw);
    HIP_TRY(hipGetLastError());
    return APZ_OK;
}

int apz_sample_moves_host(apz_engine* e, const int32_t* visits_host, int g, float temp, float alpha, float eps,
                          uint64_t seed, uint64_t step, float* pi_host, int32_t* moves_host) {
    return apz_sample_moves_keyed_host(e, visits_host, g, temp, alpha, eps, seed, step, nullptr, pi_host, moves_host);
}

int apz_sample_moves_keyed_host(apz_engine* e, const int32_t* visits_host, int g, float temp, float alpha, float eps,
                                uint64_t seed, uint64_t step, const uint64_t* keys_host, float* pi_host,
                                int32_t* moves_host) {
    if (!e || !visits_host || !pi_host || !moves_host) return fail(APZ_E_ARG, "null argument");
    if (g < 1 || e->hw > 256 || !(temp > 0.f) || !(alpha > 0.f) || eps < 0.f || eps > 1.f)
        return fail(APZ_E_ARG, "bad sampler arguments");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    const size_t hw = e->hw, vb = (size_t)g * hw * sizeof(int32_t);
    if ((size_t)g > e->smp_cap) {
        if (e->smp_vis) hipFree(e->smp_vis);
        if (e->smp_pi) hipFree(e->smp_pi);
        if (e->smp_mv) hipFree(e->smp_mv);
        if (e->smp_keys) hipFree(e->smp_keys);
        e->smp_vis = nullptr; e->smp_pi = nullptr; e->smp_mv = nullptr; e->smp_keys = nullptr; e->smp_cap = 0;
        HIP_TRY(hipMalloc((void**)&e->smp_keys, (size_t)g * sizeof(uint64_t)));
        HIP_TRY(hipMalloc((void**)&e->smp_vis, vb));
        HIP_TRY(hipMalloc((void**)&e->smp_pi, (size_t)g * hw * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&e->smp_mv, (size_t)g * sizeof(int32_t)));
        e->smp_cap = g;
    }
    HIP_TRY(hipMemcpyAsync(e->smp_vis, visits_host, vb, hipMemcpyHostToDevice, e->stream));
    if (keys_host)
        HIP_TRY(hipMemcpyAsync(e->smp_keys, keys_host, (size_t)g * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(apz::root_sample_kernel, dim3(g), dim3(64), 0, e->stream, e->smp_vis, e->smp_pi, e->smp_mv, g,
                       (int)hw, 1.0f / temp, alpha, eps, (unsigned long long)seed, (unsigned long long)step,
                       keys_host ? (const unsigned long long*)e->smp_keys : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pi_host, e->smp_pi, (size_t)g * hw * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(moves_host, e->smp_mv, (size_t)g * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return APZ_OK;
}

int64_t apz_conv3x3_packed_size(int cin_p, int cout_p) {
    if (cin_p < 1 || cout_p < 16 || cout_p % 16) return -1;
    return (int64_t)(cout_p / 16) * ((cin_p + 3) / 4) * 9 * 64;
}

// The same as apz_load_weights for tensors that already live in DEVICE memory (the trainer's): pack_all runs on `stream`
// (APZ_ENGINE_STREAM: the engine's own) without a host synchronisation, and the engine's stream waits for it.  The buffers
// are those of the engine's first apz_load_weights.
int apz_load_weights_dev(apz_engine* e, const char* const* names, const void* const* dev_ptrs, const int64_t* sizes, int n,
                         void* stream) {
    if (!e || !names || !dev_ptrs || !sizes) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    drop_forward_graphs(e);
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (!e->loaded) return fail(APZ_E_STATE, "apz_load_weights_dev refreshes a loaded engine: call apz_load_weights first");
    ParamPtrs P;
    if (int rc = check_param_table(e, names, dev_ptrs, sizes, n, P)) return rc;
    hipStream_t engine_stream = e->stream;
    StreamScope sc(e, stream);
    hipStream_t st = e->stream;
    // forwards already queued on the engine's stream still read the old weights
    if (st != engine_stream) HIP_TRY(stream_wait(e, st, engine_stream));
    // From here on packing kernels are queued on `st`: whatever happens below, the engine's stream must end up
    // ordered behind them (a half-refreshed evaluator that ALSO races the packing kernels would be worse).
    struct Closing {
        apz_engine* e;
        hipStream_t st, engine_stream;
        ~Closing() {
            if (st != engine_stream) (void)stream_wait(e, engine_stream, st);
        }
    } closing{e, st, engine_stream};
    return pack_all(e, P, st);   // (`closing` orders the engine's stream behind it: forwards queued from now on see the new weights)
}

int apz_conv3x3_pack(apz_engine* e, const void* w_dev, int cin, int cout, int transpose_flip, void* wpk_dev,
                     void* stream) {
    if (!e || !w_dev || !wpk_dev || cin < 1 || cout < 1) return fail(APZ_E_ARG, "bad argument");
    const int co_p = transpose_flip ? cin : cout;
    if (co_p % 16) return fail(APZ_E_UNSUPPORTED, "packed C_out must be a multiple of 16");
    return train_call(e, stream, [&]() -> int {
        const long total = apz_conv3x3_packed_size(transpose_flip ? cout : cin, co_p);
        hipLaunchKernelGGL(apz::pack_conv3x3_kernel, dim3((int)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0,
                           e->stream, (const float*)w_dev, (float*)wpk_dev, cin, cout, transpose_flip);
        return APZ_OK;
    });
}

int apz_conv3x3_fwd(apz_engine* e, const void* x_dev, const void* wpk_dev, const void* bias_dev, void* y_dev, int n,
                    int cin_p, int cout_p, int relu, void* stream) {
    if (!e || !x_dev || !wpk_dev || !y_dev || n < 1 || cin_p < 1) return fail(APZ_E_ARG, "bad argument");
    if (cout_p != 64 && cout_p != 128 && cout_p != 256)
        return fail(APZ_E_UNSUPPORTED, "conv3x3_fwd: C_out must be 64, 128 or 256");
    return train_call(e, stream, [&]() -> int {
        if (int rc = ensure_zeros256(e)) return rc;
        ConvLayer L;
        L.cin = cin_p;
        L.cin_pad = (cin_p + 3) / 4 * 4;
        L.cout = cout_p;
        L.residual = false;
        L.wpk = (float*)wpk_dev;
        L.bias = bias_dev ? (float*)bias_dev : e->zeros256;
        // small batches: split the output channels over 2 or 4 workgroups per board so that
        // boards x groups covers the CUs (each group stages the board's input itself)
        int groups = 1;
        while (groups * 64 < cout_p && n * groups * 2 <= e->num_cu * 2 && n * groups < e->num_cu) groups *= 2;
        const int ct = cout_p / 64 / groups;
        auto dense = [&](auto S, auto CT) {      // a square board of side S, CT tiles of 64 output channels per workgroup
            return launch_conv_r<S(), S(), CT(), false>(e, L, (const float*)x_dev, nullptr, (float*)y_dev, n, S() * S(), S(), relu,
                                                        groups);
        };
        auto board = [&](auto S) { return ct == 1 ? dense(S, int_c<1>{}) : ct == 2 ? dense(S, int_c<2>{}) : dense(S, int_c<4>{}); };
        const int H = e->cfg.height, W = e->cfg.width;
        const int rc = H == 15 && W == 15 ? board(int_c<15>{}) : H == 8 && W == 8 ? board(int_c<8>{}) : APZ_E_UNSUPPORTED;
        L.wpk = nullptr;
        L.bias = nullptr;
        if (rc == APZ_E_UNSUPPORTED) return fail(rc, "conv3x3_fwd: unsupported board size");
        return rc;
    });
}

int apz_conv15h_fwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* bias_dev, const void* resid_dev,
                    void* y_dev, int n, int cin, int cout, int relu, void* flag_dev, void* stream) {
    if (!e || !x_dev || !w_dev || !y_dev || !flag_dev || n < 1 || cin < 1 || cout < 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "conv15h_fwd: 15x15 boards only");
    if (!apz::Conv15H::supports(cin, cout))
        return fail(APZ_E_UNSUPPORTED, "conv15h_fwd: C_in must be a multiple of 64 and C_out a multiple of 16, not " +
                                           std::to_string(cin) + " -> " + std::to_string(cout));
    if ((int64_t)cin * apz::Conv15H::HW * 4 > 0x7fffffffLL || (int64_t)n * (cout / 16) > 0x7fffffffLL)
        return fail(APZ_E_UNSUPPORTED, "conv15h_fwd: too many channels or items for one launch");
    return train_call(e, stream, [&]() -> int {
        // [scale cout][shift cout] doubles, [bias][1 / S] floats, the packed weights (16-byte aligned: cout is a multiple of 16)
        const size_t fold_bytes = 2 * (size_t)cout * sizeof(double), bias_bytes = 2 * (size_t)cout * sizeof(float);
        if (int rc = e->conv15h_scratch.reserve(fold_bytes + bias_bytes + apz::Conv8H::pk_bytes(cin, cout))) return rc;
        char* base = e->conv15h_scratch.as<char>();
        double* scale = (double*)base;
        ConvLayer L;
        L.cin = cin;
        L.cout = cout;
        L.bias8h = (float*)(base + fold_bytes);
        L.wpk8h = base + fold_bytes + bias_bytes;
        hipLaunchKernelGGL(apz::conv15h_plain_fold_kernel, dim3((cout + 63) / 64), dim3(64), 0, e->stream, (const float*)bias_dev,
                           scale, scale + cout, cout);
        hipLaunchKernelGGL(apz::pack_conv8h_kernel, dim3(cout), dim3(256), 0, e->stream, (const float*)w_dev, scale, scale + cout,
                           (unsigned short*)L.wpk8h, L.bias8h, cin, cout);
        HIP_TRY(hipGetLastError());
        const int rc = with_flag(resid_dev != nullptr, [&](auto RESID) {
            return launch_conv15h_t<RESID()>(e, L, (const float*)x_dev, (const float*)resid_dev, (float*)y_dev, n, relu != 0,
                                             (unsigned*)flag_dev);
        });
        L.wpk8h = nullptr;        // the scratch buffer's, not the layer's
        L.bias8h = nullptr;
        return rc;
    });
}

// ---- the training step of the generic 15x15 nets on conv15h_kernel (HipTrainer(trunk_arith="f16x2"), csrc/conv15_split.h)
int64_t apz_conv15h_packed_size(int cin, int cout) {
    if (cin < 1 || cout < 1 || !apz::Conv15H::supports(cin, cout)) return fail(APZ_E_ARG, "bad argument");
    return (int64_t)(apz::Conv8H::pk_bytes(cin, cout) / 4);
}

namespace {
int conv15h_packed_check(const apz_engine* e, const void* x, const void* pk, const void* bias8h, const void* y, const void* flag,
                         int n, int cin, int cout, const char* who) {
    if (!e || !x || !pk || !bias8h || !y || !flag || n < 1 || cin < 1 || cout < 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, std::string(who) + ": 15x15 boards only");
    if (!apz::Conv15H::supports(cin, cout))
        return fail(APZ_E_UNSUPPORTED, std::string(who) + ": C_in must be a multiple of 64 and C_out a multiple of 16, not " +
                                           std::to_string(cin) + " -> " + std::to_string(cout));
    if ((int64_t)cin * apz::Conv15H::HW * 4 > 0x7fffffffLL || (int64_t)n * (cout / 16) > 0x7fffffffLL)
        return fail(APZ_E_UNSUPPORTED, std::string(who) + ": too many channels or items for one launch");
    return APZ_OK;
}
}  // namespace

int apz_conv15h_fwd_packed(apz_engine* e, const void* x_dev, const void* pk_dev, const void* bias8h_dev, const void* resid_dev,
                           void* y_dev, int n, int cin, int cout, void* flag_dev, void* stream) {
    if (int rc = conv15h_packed_check(e, x_dev, pk_dev, bias8h_dev, y_dev, flag_dev, n, cin, cout, "conv15h_fwd_packed")) return rc;
    return train_call(e, stream, [&]() -> int {
        ConvLayer L;
        L.cin = cin;
        L.cout = cout;
        L.bias8h = (float*)const_cast<void*>(bias8h_dev);
        L.wpk8h = const_cast<void*>(pk_dev);
        const int rc = with_flag(resid_dev != nullptr, [&](auto RESID) {
            return launch_conv15h_t<RESID()>(e, L, (const float*)x_dev, (const float*)resid_dev, (float*)y_dev, n, 0,
                                             (unsigned*)flag_dev);
        });
        L.wpk8h = nullptr;        // the caller's, not the layer's
        L.bias8h = nullptr;
        return rc;
    });
}

int apz_conv15h_dgrad(apz_engine* e, const void* dy_dev, const void* pk_dev, const void* bias8h_dev, const void* add_dev,
                      void* dx_dev, int n, int c_dy, int c_dx, const void* dymax_dev, int dymax_count, void* flag_dev,
                      void* stream) {
    if (!dymax_dev || dymax_count < 1) return fail(APZ_E_ARG, "bad argument");
    if (int rc = conv15h_packed_check(e, dy_dev, pk_dev, bias8h_dev, dx_dev, flag_dev, n, c_dy, c_dx, "conv15h_dgrad")) return rc;
    using T = apz::Conv15H;
    return train_call(e, stream, [&]() -> int {
        const int grid = (int)T::grid_for((long)n * (c_dx / 16), e->num_cu);
        return with_flag(add_dev != nullptr, [&](auto RESID) -> int {
            const auto kern = apz::conv15h_kernel<RESID(), apz::CONV15H_DGRAD, const float*, int>;
            if (int rc = need_lds(e, (const void*)kern, T::LDS_BYTES)) return rc;
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), T::LDS_BYTES, e->stream, (const float*)dy_dev, pk_dev,
                               (const float*)bias8h_dev, (const float*)add_dev, (float*)dx_dev, n, c_dy, c_dx, 0, (unsigned*)flag_dev,
                               (const float*)dymax_dev, dymax_count);
            HIP_TRY(hipGetLastError());
            return APZ_OK;
        });
    });
}

int64_t apz_wino_packed_size(void) { return (int64_t)apz::WinoPack::UPK_FLOATS; }

int apz_wino_pack(apz_engine* e, const void* w_dev, int transpose_flip, void* upk_dev, void* stream) {
    if (!e || !w_dev || !upk_dev) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        hipLaunchKernelGGL(apz::pack_wino2_kernel, dim3(8 * 2 * 32 * 64 / 256), dim3(256), 0, e->stream, (const float*)w_dev,
                           (float*)upk_dev, transpose_flip);
        return APZ_OK;
    });
}

int apz_wino_pack_many(apz_engine* e, const void* w_dev, int count, void* upk_dev, void* stream) {
    if (!e || !w_dev || !upk_dev || count < 1 || count > 16384) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        hipLaunchKernelGGL(apz::pack_wino2_many_kernel, dim3(8 * 2 * 32 * 64 / 256, 2 * count), dim3(256), 0, e->stream,
                           (const float*)w_dev, (float*)upk_dev);
        return APZ_OK;
    });
}

int apz_wino_conv_add(apz_engine* e, const void* x_dev, const void* upk_dev, const void* bias_dev, const void* resid_dev,
                      void* y_dev, int n, int relu, int layout, void* stream) {
    if (!e || !x_dev || !upk_dev || !y_dev || n < 1 || layout < 0 || layout > 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "wino_conv: 15x15 boards only");
    if (resid_dev && layout != APZ_LAYOUT_ROWS16) return fail(APZ_E_UNSUPPORTED, "wino_conv: residual input in the padded-row layout only");
    return train_call(e, stream, [&]() -> int {
        if (int rc = ensure_zeros256(e)) return rc;
        const long planes = (long)n * 128;
        const int cgrid = (int)std::min<long>((planes * 240 + 255) / 256, 16384);
        const bool dense = layout == APZ_LAYOUT_DENSE;
        if (dense)      // the rows16 copies of input and output
            for (auto& buf : e->wino_scratch)
                if (int rc = buf.reserve((size_t)planes * 240 * sizeof(float))) return rc;
        const float* xin = dense ? e->wino_scratch[0].as<float>() : (const float*)x_dev;
        float* yout = dense ? e->wino_scratch[1].as<float>() : (float*)y_dev;
        if (dense)
            hipLaunchKernelGGL(apz::rows16_from_dense_kernel, dim3(cgrid), dim3(256), 0, e->stream, (const float*)x_dev,
                               e->wino_scratch[0].as<float>(), planes);
        const float* b = bias_dev ? (const float*)bias_dev : e->zeros256;
        const float* rs = (const float*)resid_dev;
        // the self-play path's kernel (csrc/trunk15_wino3.h)
        if (int rc = with_flag(rs != nullptr, [&](auto RESID) {
                return with_flag(relu != 0, [&](auto RELU) {
                    return launch_wino3_t<RESID(), RELU()>(e, xin, (const float*)upk_dev, b, rs, yout, n);
                });
            }))
            return rc;
        if (dense)
            hipLaunchKernelGGL(apz::rows16_to_dense_kernel, dim3(cgrid), dim3(256), 0, e->stream, yout, (float*)y_dev, planes);
        return APZ_OK;
    });
}

int apz_wino_conv_stats(apz_engine* e, const void* x_dev, const void* upk_dev, const void* bias_dev, void* y_dev,
                        void* stats_dev, int n, void* stream) {
    if (!e || !x_dev || !upk_dev || !y_dev || !stats_dev || n < 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "wino_conv: 15x15 boards only");
    if (n > WINO3_MAX_BOARDS) return fail(APZ_E_UNSUPPORTED, "wino_conv_stats: one launch (<= 16384 boards)");
    using T = apz::Wino3;
    return train_call(e, stream, [&]() -> int {
        if (int rc = ensure_zeros256(e)) return rc;
        const float* b = bias_dev ? (const float*)bias_dev : e->zeros256;
        bool quarter = false;
        const int grid = apz::wino3_grid(n, e->num_cu, e->no_quarter_trunk ? nullptr : &quarter);
        return with_flag(quarter, [&](auto QUARTER) -> int {
            const auto kern = apz::trunk15_wino3_kernel<false, false, QUARTER(), true>;
            if (int rc = need_lds(e, (const void*)kern, T::LDS_BYTES)) return rc;
            hipLaunchKernelGGL(kern, dim3(grid), dim3(512), T::LDS_BYTES, e->stream, (const float*)x_dev, (const float*)upk_dev, b,
                               (const float*)stats_dev, (float*)y_dev, n);
            return APZ_OK;
        });
    });
}

int apz_wino_conv(apz_engine* e, const void* x_dev, const void* upk_dev, const void* bias_dev, void* y_dev, int n, int relu,
                  int layout, void* stream) {
    return apz_wino_conv_add(e, x_dev, upk_dev, bias_dev, nullptr, y_dev, n, relu, layout, stream);
}

// ---- the training step's trunk on the f16x2 kernel (csrc/trunk15_wino3h16.h, trunk15_wino3h16_train_kernel)
int64_t apz_wino3h_packed_size(void) { return (int64_t)(apz::Wino3H16::UPK_BYTES / 4); }

int apz_wino3h_pack_many(apz_engine* e, const void* w_dev, const void* b_dev, int count, void* upk_dev, void* bias_dev,
                         void* flag_dev, void* stream) {
    if (!e || !w_dev || !upk_dev || !bias_dev || count < 1 || count > 16384) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        hipLaunchKernelGGL(apz::pack_wino3h16_many_kernel, dim3(128, 2 * count), dim3(128), 0, e->stream, (const float*)w_dev,
                           (const float*)b_dev, (unsigned short*)upk_dev, (float*)bias_dev, (unsigned*)flag_dev);
        return APZ_OK;
    });
}

extern "C++" {
namespace {
template <int FORM, bool RESID>
int launch_wino3h16_train(apz_engine* e, const void* x_dev, const void* upk_dev, const void* bias_dev,
                          const void* resid_dev, void* y_dev, int n, void* flag_dev, void* aux, int aux_n, void* stream) {
    if (!e || !x_dev || !upk_dev || !bias_dev || !y_dev || !aux || n < 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "wino3h: 15x15 boards only");
    if (n > WINO3_MAX_BOARDS) return fail(APZ_E_UNSUPPORTED, "wino3h: one launch (<= 16384 boards)");
    using T = apz::Wino3H16;
    const auto kern = apz::trunk15_wino3h16_kernel<RESID, false, FORM>;
    return train_call(e, stream, [&]() -> int {
        if (int rc = need_lds(e, (const void*)kern, T::LDS_BYTES)) return rc;
        hipLaunchKernelGGL(kern, dim3(apz::wino3_grid(n, e->num_cu)), dim3(512), T::LDS_BYTES, e->stream, (const float*)x_dev,
                           upk_dev, (const float*)bias_dev, (const float*)resid_dev, (float*)y_dev, n, (unsigned*)flag_dev, aux,
                           aux_n);
        return APZ_OK;
    });
}
}  // namespace
}  // extern "C++"

int apz_wino3h_conv_stats(apz_engine* e, const void* x_dev, const void* upk_dev, const void* bias_dev, void* y_dev,
                          void* stats_dev, int n, void* flag_dev, void* stream) {
    return launch_wino3h16_train<apz::WINO3H16_STATS, false>(e, x_dev, upk_dev, bias_dev, nullptr, y_dev, n, flag_dev,
                                                             stats_dev, 0, stream);
}

int apz_wino3h_conv_dgrad(apz_engine* e, const void* dy_dev, const void* upk_dev, const void* bias_dev, const void* add_dev,
                          void* dx_dev, int n, const void* dymax_dev, int dymax_count, void* flag_dev, void* stream) {
    if (dymax_count < 1) return fail(APZ_E_ARG, "bad argument");
    return with_flag(add_dev != nullptr, [&](auto RESID) {
        return launch_wino3h16_train<apz::WINO3H16_DGRAD, RESID()>(e, dy_dev, upk_dev, bias_dev, add_dev, dx_dev, n, flag_dev,
                                                                   const_cast<void*>(dymax_dev), dymax_count, stream);
    });
}

int apz_conv3x3_wgrad(apz_engine* e, const void* x_dev, const void* dy_dev, void* dw_dev, int n, int cin, int cout,
                      int layout, void* stream) {
    if (!e || !x_dev || !dy_dev || !dw_dev || n < 1 || cin < 1 || cout < 32 || cout % 32 || layout < 0 || layout > 1)
        return fail(APZ_E_ARG, "bad argument (C_out must be a multiple of 32)");
    if (layout == APZ_LAYOUT_ROWS16 && (e->cfg.height != 15 || e->cfg.width != 15))
        return fail(APZ_E_UNSUPPORTED, "padded-row layout: 15x15 boards only");
    return train_call(e, stream, [&]() -> int {
        const int gx = cout / 32, gy = (cin + 63) / 64;
        // a square board of side S (R16: in padded rows), `per_cu` workgroups per CU: every slice of the batch leaves its
        // partial sums, which are then added in index order
        auto run = [&](auto S, auto R16, int per_cu) -> int {
            using G = apz::WgradGeo<S(), S(), R16()>;
            const auto kern = apz::conv3x3_wgrad_kernel<S(), S(), R16()>;
            const int slices = std::max(1, std::min(n, (e->num_cu * per_cu) / std::max(1, gx * gy)));
            if (int rc = e->wgw_scratch.reserve((size_t)slices * cout * cin * 9 * sizeof(float))) return rc;
            if (int rc = need_lds(e, (const void*)kern, G::LDS_BYTES)) return rc;
            hipLaunchKernelGGL(kern, dim3(gx, gy, slices), dim3(256), G::LDS_BYTES, e->stream, (const float*)x_dev,
                               (const float*)dy_dev, e->wgw_scratch.as<float>(), n, cin, cout);
            hipLaunchKernelGGL(apz::colsum_kernel, dim3((cout * cin * 9 + 63) / 64), dim3(256), 0, e->stream,
                               e->wgw_scratch.as<const float>(), (float*)dw_dev, slices, cout * cin * 9, 1.0f);
            return APZ_OK;
        };
        const int H = e->cfg.height, W = e->cfg.width;
        if (H == 15 && W == 15)     // 85 KB LDS: one workgroup per CU
            return with_flag(layout == APZ_LAYOUT_ROWS16, [&](auto R16) { return run(int_c<15>{}, R16, 1); });
        if (H == 8 && W == 8) return run(int_c<8>{}, std::false_type{}, 2);
        return fail(APZ_E_UNSUPPORTED, "conv3x3_wgrad: unsupported board size");
    });
}

namespace {
int bn_geometry(apz_engine* e, int layout, int* ps, int* rs) {
    const int H = e->cfg.height, W = e->cfg.width;
    if (layout == APZ_LAYOUT_DENSE) {
        *ps = H * W, *rs = W;
    } else if (layout == APZ_LAYOUT_ROWS16 && H == 15 && W == 15) {
        *ps = 240, *rs = 16;
    } else {
        return fail(APZ_E_UNSUPPORTED, "padded-row layout: 15x15 boards only");
    }
    return APZ_OK;
}
constexpr int BN_SPLITS = 64;      // batch splits per channel at most (every consumer workgroup adds them)
// per-(channel, split) partial sums: overwritten by every statistics launch, nothing to zero
int bn_scratch(apz_engine* e) { return e->bn_part.reserve((size_t)256 * BN_SPLITS * 2 * sizeof(double)); }
// grid.y of the four BatchNorm launches: channels x splits ~ 8 workgroups per CU (padded rows: four boards per trip)
int bn_splits(const apz_engine* e, int n, int C, int layout) {
    const int per = layout == APZ_LAYOUT_ROWS16 ? (n + 3) / 4 : n;
    return std::max(1, std::min({per, (e->num_cu * (layout == APZ_LAYOUT_ROWS16 ? 8 : 4)) / C, BN_SPLITS}));
}
// framed boards in the training step (csrc/bn_frame.h, csrc/frame15.h): a board of side S on the 15x15 engine
int frame_train_check(const apz_engine* e, int side, const char* who) {
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, std::string(who) + ": the 15x15 engine only");
    if (!(apz::Frame15::framed_side(side) || side == 15))
        return fail(APZ_E_UNSUPPORTED, std::string(who) + ": side must be 6, 7, 9, 11, 12, 13, 14 or 15");
    return APZ_OK;
}

// The BatchNorm forward on checked arguments: scratch, splits, the statistics launch and the apply launch.  side 0: the
// engine's board in `layout` (ps, rs from bn_geometry); else a framed board on padded rows (csrc/bn_frame.h): count n side side.
int bn_fwd_launch(apz_engine* e, const void* x_dev, const void* resid_dev, const void* gamma_dev, const void* beta_dev,
                  void* run_mean_dev, void* run_var_dev, void* y_dev, void* mean_dev, void* invstd_dev, const void* stats_dev,
                  void* mask_dev, int n, int C, int layout, int relu, float momentum, float eps, int side, int ps, int rs,
                  void* stream) {
    return train_call(e, stream, [&]() -> int {
        if (int rc = bn_scratch(e)) return rc;
        double* part = e->bn_part.as<double>();
        const int H = side ? side : e->cfg.height, W = side ? side : e->cfg.width;
        const int splits = bn_splits(e, n, C, layout);
        const apz::BnFinal fin{(float*)mean_dev, (float*)invstd_dev, (float*)run_mean_dev, (float*)run_var_dev, (double)n * H * W, eps,
                               momentum};
        auto rows = [&](auto board) {
            using B = decltype(board);
            // statistics from the producer (apz_wino_conv_stats: one pair of sums per channel and board): no pass over x for them
            if (!stats_dev)
                hipLaunchKernelGGL(apz::bn_stats_rows_kernel<B>, dim3(C, splits), dim3(256), 0, e->stream, (const float*)x_dev, part,
                                   n, C, board);
            hipLaunchKernelGGL(apz::bn_apply_rows_kernel<B>, dim3(C, splits), dim3(256), 0, e->stream, (const float*)x_dev,
                               (const float*)resid_dev, (const float*)gamma_dev, (const float*)beta_dev,
                               stats_dev ? (const double*)stats_dev : part, stats_dev ? n : splits, fin, (float*)y_dev,
                               (unsigned char*)mask_dev, n, C, relu, board);
        };
        if (side) {
            rows(apz::BoardFrame{side});
        } else if (layout == APZ_LAYOUT_ROWS16) {
            rows(apz::Board15{});
        } else {
            hipLaunchKernelGGL(apz::bn_stats_kernel, dim3(C, splits), dim3(256), 0, e->stream, (const float*)x_dev, part, n, C, ps,
                               rs, H, W);
            hipLaunchKernelGGL(apz::bn_apply_kernel, dim3(C, splits), dim3(256), 0, e->stream, (const float*)x_dev,
                               (const float*)resid_dev, (const float*)gamma_dev, (const float*)beta_dev, part, splits, fin,
                               (float*)y_dev, n, C, ps, rs, H, W, relu);
        }
        return APZ_OK;
    });
}

// ... and the backward: the reduce launch and the apply launch
int bn_bwd_launch(apz_engine* e, const void* dy_dev, const void* x_dev, const void* out_dev, const void* mask_dev,
                  const void* gamma_dev, const void* mean_dev, const void* invstd_dev, void* dx_dev, void* dres_dev,
                  void* dgamma_dev, void* dbeta_dev, void* dxsum_dev, int dxsum_ld, void* dxmax_dev, int n, int C, int layout,
                  int relu, int side, int ps, int rs, void* stream) {
    return train_call(e, stream, [&]() -> int {
        if (int rc = bn_scratch(e)) return rc;
        double* part = e->bn_part.as<double>();
        const int H = side ? side : e->cfg.height, W = side ? side : e->cfg.width;
        const int splits = bn_splits(e, n, C, layout);
        auto rows = [&](auto board) {
            using B = decltype(board);
            hipLaunchKernelGGL(apz::bn_bwd_reduce_rows_kernel<B>, dim3(C, splits), dim3(256), 0, e->stream, (const float*)dy_dev,
                               (const float*)x_dev, (const float*)out_dev, (const float*)mean_dev, (const float*)invstd_dev, part,
                               (const unsigned char*)mask_dev, n, C, relu, board);
            hipLaunchKernelGGL(apz::bn_bwd_apply_rows_kernel<B>, dim3(C, splits), dim3(256), 0, e->stream, (const float*)dy_dev,
                               (const float*)x_dev, (const float*)out_dev, (const float*)gamma_dev, (const float*)mean_dev,
                               (const float*)invstd_dev, part, splits, (float*)dx_dev, (float*)dres_dev, (float*)dgamma_dev,
                               (float*)dbeta_dev, (float*)dxsum_dev, dxsum_ld, (const unsigned char*)mask_dev, n, C, relu,
                               (double)n * H * W, (float*)dxmax_dev, board);
        };
        if (side) {
            rows(apz::BoardFrame{side});
        } else if (layout == APZ_LAYOUT_ROWS16) {
            rows(apz::Board15{});
        } else {
            hipLaunchKernelGGL(apz::bn_bwd_reduce_kernel, dim3(C, splits), dim3(256), 0, e->stream, (const float*)dy_dev,
                               (const float*)x_dev, (const float*)out_dev, (const float*)mean_dev, (const float*)invstd_dev, part,
                               n, C, ps, rs, H, W, relu);
            hipLaunchKernelGGL(apz::bn_bwd_apply_kernel, dim3(C, splits), dim3(256), 0, e->stream, (const float*)dy_dev,
                               (const float*)x_dev, (const float*)out_dev, (const float*)gamma_dev, (const float*)mean_dev,
                               (const float*)invstd_dev, part, splits, (float*)dx_dev, (float*)dres_dev, (float*)dgamma_dev,
                               (float*)dbeta_dev, (float*)dxsum_dev, dxsum_ld, n, C, ps, rs, H, W, relu, (double)n * H * W,
                               (float*)dxmax_dev);
        }
        return APZ_OK;
    });
}
}  // namespace

int apz_bn_fwd(apz_engine* e, const void* x_dev, const void* resid_dev, const void* gamma_dev, const void* beta_dev,
               void* run_mean_dev, void* run_var_dev, void* y_dev, void* mean_dev, void* invstd_dev, int n, int C, int layout,
               int relu, float momentum, float eps, void* stream) {
    return apz_bn_fwd_stats(e, x_dev, resid_dev, gamma_dev, beta_dev, run_mean_dev, run_var_dev, y_dev, mean_dev, invstd_dev,
                            nullptr, nullptr, n, C, layout, relu, momentum, eps, stream);
}

int apz_bn_fwd_stats(apz_engine* e, const void* x_dev, const void* resid_dev, const void* gamma_dev, const void* beta_dev,
                     void* run_mean_dev, void* run_var_dev, void* y_dev, void* mean_dev, void* invstd_dev,
                     const void* stats_dev, void* mask_dev, int n, int C, int layout, int relu, float momentum, float eps,
                     void* stream) {
    if (!e || !x_dev || !beta_dev || !y_dev || !mean_dev || !invstd_dev || n < 1 || C < 1 || C > 256)
        return fail(APZ_E_ARG, "bad argument");
    if ((stats_dev || mask_dev) && layout != APZ_LAYOUT_ROWS16) return fail(APZ_E_UNSUPPORTED, "bn_fwd_stats: padded-row layout only");
    int ps, rs;
    if (int rc = bn_geometry(e, layout, &ps, &rs)) return rc;
    return bn_fwd_launch(e, x_dev, resid_dev, gamma_dev, beta_dev, run_mean_dev, run_var_dev, y_dev, mean_dev, invstd_dev, stats_dev,
                         mask_dev, n, C, layout, relu, momentum, eps, 0, ps, rs, stream);
}

int apz_bn_bwd_splits(apz_engine* e, int n, int C, int layout) {
    if (!e || n < 1 || C < 1 || C > 256 || layout < 0 || layout > 1) return fail(APZ_E_ARG, "bad argument");
    return bn_splits(e, n, C, layout);
}

int apz_bn_bwd(apz_engine* e, const void* dy_dev, const void* x_dev, const void* out_dev, const void* mask_dev,
               const void* gamma_dev, const void* mean_dev, const void* invstd_dev, void* dx_dev, void* dres_dev, void* dgamma_dev,
               void* dbeta_dev, void* dxsum_dev, int dxsum_ld, int n, int C, int layout, int relu, void* stream) {
    return apz_bn_bwd_max(e, dy_dev, x_dev, out_dev, mask_dev, gamma_dev, mean_dev, invstd_dev, dx_dev, dres_dev, dgamma_dev,
                          dbeta_dev, dxsum_dev, dxsum_ld, nullptr, n, C, layout, relu, stream);
}

int apz_bn_bwd_max(apz_engine* e, const void* dy_dev, const void* x_dev, const void* out_dev, const void* mask_dev,
                   const void* gamma_dev, const void* mean_dev, const void* invstd_dev, void* dx_dev, void* dres_dev,
                   void* dgamma_dev, void* dbeta_dev, void* dxsum_dev, int dxsum_ld, void* dxmax_dev, int n, int C, int layout,
                   int relu, void* stream) {
    if (!e || !dy_dev || !x_dev || !mean_dev || !invstd_dev || !dx_dev || n < 1 || C < 1 || C > 256 ||
        (relu && !out_dev && !mask_dev) || (dxsum_dev && dxsum_ld < C) || (mask_dev && layout != APZ_LAYOUT_ROWS16))
        return fail(APZ_E_ARG, "bad argument");
    // the maxima feed the f16x2 data gradients, which exist on 15x15 boards only: padded rows (trunk15_wino3h16.h) and, dense,
    // the generic nets (conv15_split.h); a dense 8x8 tensor has no consumer for them and keeps its refusal
    if (dxmax_dev && layout != APZ_LAYOUT_ROWS16 && (e->cfg.height != 15 || e->cfg.width != 15))
        return fail(APZ_E_UNSUPPORTED, "bn_bwd_max: padded-row layout only");
    int ps, rs;
    if (int rc = bn_geometry(e, layout, &ps, &rs)) return rc;
    return bn_bwd_launch(e, dy_dev, x_dev, out_dev, mask_dev, gamma_dev, mean_dev, invstd_dev, dx_dev, dres_dev, dgamma_dev,
                         dbeta_dev, dxsum_dev, dxsum_ld, dxmax_dev, n, C, layout, relu, 0, ps, rs, stream);
}

// ... on framed boards: the same launches with the board mask (no statistics from a convolution's epilogue: those cover
// all 225 cells)
int apz_bn_fwd_frame(apz_engine* e, const void* x_dev, const void* resid_dev, const void* gamma_dev, const void* beta_dev,
                     void* run_mean_dev, void* run_var_dev, void* y_dev, void* mean_dev, void* invstd_dev, void* mask_dev, int n,
                     int C, int layout, int relu, float momentum, float eps, int side, void* stream) {
    if (!e || !x_dev || !beta_dev || !y_dev || !mean_dev || !invstd_dev || n < 1 || C < 1 || C > 256)
        return fail(APZ_E_ARG, "bad argument");
    if (layout != APZ_LAYOUT_ROWS16) return fail(APZ_E_UNSUPPORTED, "bn_fwd_frame: padded-row layout only");
    if (int rc = frame_train_check(e, side, "bn_fwd_frame")) return rc;
    return bn_fwd_launch(e, x_dev, resid_dev, gamma_dev, beta_dev, run_mean_dev, run_var_dev, y_dev, mean_dev, invstd_dev, nullptr,
                         mask_dev, n, C, layout, relu, momentum, eps, side, 0, 0, stream);
}

int apz_bn_bwd_frame(apz_engine* e, const void* dy_dev, const void* x_dev, const void* out_dev, const void* mask_dev,
                     const void* gamma_dev, const void* mean_dev, const void* invstd_dev, void* dx_dev, void* dres_dev,
                     void* dgamma_dev, void* dbeta_dev, void* dxsum_dev, int dxsum_ld, void* dxmax_dev, int n, int C, int layout,
                     int relu, int side, void* stream) {
    if (!e || !dy_dev || !x_dev || !mean_dev || !invstd_dev || !dx_dev || n < 1 || C < 1 || C > 256 ||
        (relu && !out_dev && !mask_dev) || (dxsum_dev && dxsum_ld < C))
        return fail(APZ_E_ARG, "bad argument");
    if (layout != APZ_LAYOUT_ROWS16) return fail(APZ_E_UNSUPPORTED, "bn_bwd_frame: padded-row layout only");
    if (int rc = frame_train_check(e, side, "bn_bwd_frame")) return rc;
    return bn_bwd_launch(e, dy_dev, x_dev, out_dev, mask_dev, gamma_dev, mean_dev, invstd_dev, dx_dev, dres_dev, dgamma_dev,
                         dbeta_dev, dxsum_dev, dxsum_ld, dxmax_dev, n, C, layout, relu, side, 0, 0, stream);
}

int apz_colsum(apz_engine* e, const void* in_dev, void* out_dev, int rows, int cols, float scale, void* stream) {
    if (!e || !in_dev || !out_dev || rows < 1 || cols < 1) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        hipLaunchKernelGGL(apz::colsum_kernel, dim3((cols + 63) / 64), dim3(256), 0, e->stream, (const float*)in_dev, (float*)out_dev,
                           rows, cols, scale);
        return APZ_OK;
    });
}

extern "C++" {
namespace {
// Both Winograd weight-gradient entry points (T = apz::WgradWino3 / apz::WgradWino3H; `kernel(BUF)` = T's kernel with or
// without raw buffer loads; `extra...` = the kernel's arguments behind spx): the decomposition by channel blocks
// (csrc/wgrad_wino3.h: 16 blocks x slices = one workgroup per CU; the workgroups of a slice sit on one XCD, see the
// kernel), the slices' scratch, the launch, and the second launch that sums the slices' partial dU and transforms the sum
// back into dw.
template <class T, class K, class... A>
int wgrad_wino_call(apz_engine* e, K kernel, const void* x_dev, const void* dy_dev, void* dw_dev, int n, void* stream, A... extra) {
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "wgrad_wino: 15x15 boards only");
    if (n > 32768) return fail(APZ_E_UNSUPPORTED, "wgrad_wino: at most 32768 boards per call (32-bit buffer offsets)");
    return train_call(e, stream, [&]() -> int {
        const int spx = std::max(1, std::min((n + 7) / 8, e->num_cu / (8 * T::BLOCKS)));
        const int slices = 8 * spx;
        if (int rc = e->wgw_scratch.reserve((size_t)slices * apz::WgradWino::SCRATCH_FLOATS_PER_SLICE * sizeof(float))) return rc;
        float* part = e->wgw_scratch.as<float>();
        // rows through raw buffer loads (hardware zero fill for rows off the board, scalar board offset) from 256 boards on:
        // 133.6 against 144.4 us at 512 boards, 38.7 against 37.8 us at 128 (same box, alternating rounds: tools/wgrad_kernel_bench.hip)
        if (int rc = with_flag(n >= 256, [&](auto BUF) -> int {
                const auto kern = kernel(BUF);
                if (int rc = need_lds(e, (const void*)kern, T::LDS_BYTES)) return rc;
                hipLaunchKernelGGL(kern, dim3(T::BLOCKS * slices), dim3(T::THREADS), T::LDS_BYTES, e->stream, (const float*)x_dev,
                                   (const float*)dy_dev, part, n, spx, extra...);
                return APZ_OK;
            }))
            return rc;
        hipLaunchKernelGGL(apz::wgrad_wino_finish_kernel, dim3(128 * 128 * 9 / 4 / 256), dim3(256), 0, e->stream, (const float*)part,
                           slices, (float*)dw_dev);
        return APZ_OK;
    });
}
}  // namespace
}  // extern "C++"

int apz_wgrad_wino(apz_engine* e, const void* x_dev, const void* dy_dev, void* dw_dev, int n, void* stream) {
    if (!e || !x_dev || !dy_dev || !dw_dev || n < 1) return fail(APZ_E_ARG, "bad argument");
    return wgrad_wino_call<apz::WgradWino3>(e, [](auto BUF) { return apz::wgrad_wino3_kernel<BUF()>; }, x_dev, dy_dev, dw_dev, n,
                                            stream);
}

int apz_wgrad_wino_f16x2(apz_engine* e, const void* x_dev, const void* dy_dev, void* dw_dev, int n, const void* dymax_dev,
                         int dymax_count, void* flag_dev, void* stream) {
    if (!e || !x_dev || !dy_dev || !dw_dev || !dymax_dev || dymax_count < 1 || n < 1) return fail(APZ_E_ARG, "bad argument");
    return wgrad_wino_call<apz::WgradWino3H>(e, [](auto BUF) { return apz::wgrad_wino3h_kernel<BUF()>; }, x_dev, dy_dev, dw_dev, n,
                                             stream, (const float*)dymax_dev, dymax_count, (unsigned*)flag_dev);
}

extern "C++" {
namespace {
// A host table of `count` T (the optimiser's and the average's tensor entries, the gather's entry words) into the device
// buffer the next launch reads it from, inside a train_call -> *dev.  Stream-ordered: the copy queues behind the previous
// launch that read the same buffer, and for pageable host memory hipMemcpyAsync returns once the few KB have been staged, so
// the caller's table need not outlive the call.  (No stream synchronisation: the optimiser step does not drain the GPU.)
template <class T>
int upload_table(apz_engine* e, DeviceBuffer& buf, const void* table_host, int count, const T** dev) {
    const size_t bytes = (size_t)count * sizeof(T);
    if (int rc = buf.reserve(bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(buf, table_host, bytes, hipMemcpyHostToDevice, e->stream));
    *dev = buf.as<const T>();
    return APZ_OK;
}
}  // namespace
}  // extern "C++"

// (csrc/conv15_split.h, pack_conv15h_many_kernel: the table goes the way of the optimiser's)
int apz_conv15h_pack_many(apz_engine* e, const void* table_host, int count, void* flag_dev, void* stream) {
    if (!e || !table_host || count < 1 || count > 4096) return fail(APZ_E_ARG, "bad argument");
    static_assert(sizeof(apz::Conv15HPackEntry) == 56, "apz_conv15h_pack_entry layout");
    const apz::Conv15HPackEntry* host = (const apz::Conv15HPackEntry*)table_host;
    int maxc = 0;
    for (int i = 0; i < count; i++) {
        const apz::Conv15HPackEntry& E = host[i];
        if (!E.w || !E.pk[0] || !E.pk[1] || !E.bias8h[0] || !E.bias8h[1] || E.cin < 1 || E.cout < 1)
            return fail(APZ_E_ARG, "bad argument");
        // both orientations run on the kernel: C_in -> C_out and C_out -> C_in
        if (E.cin % 64 || E.cout % 64 || E.cin > 65536 || E.cout > 65536)
            return fail(APZ_E_UNSUPPORTED, "conv15h_pack_many: C_in and C_out must be multiples of 64, not " + std::to_string(E.cin) +
                                               " -> " + std::to_string(E.cout));
        maxc = std::max(maxc, std::max(E.cin, E.cout));
    }
    return train_call(e, stream, [&]() -> int {
        const apz::Conv15HPackEntry* tab;
        if (int rc = upload_table(e, e->conv15h_tab, table_host, count, &tab)) return rc;
        hipLaunchKernelGGL(apz::pack_conv15h_many_kernel, dim3(maxc, 2 * count), dim3(256), 0, e->stream, tab, (unsigned*)flag_dev);
        HIP_TRY(hipGetLastError());
        return APZ_OK;
    });
}

int apz_adam_step(apz_engine* e, const void* table_host, int ntensors, float lr_t, float b1, float b2, float eps,
                  float rescale, void* stream) {
    return apz_adam_step_unless(e, table_host, ntensors, lr_t, b1, b2, eps, rescale, nullptr, stream);
}

int apz_adam_step_unless(apz_engine* e, const void* table_host, int ntensors, float lr_t, float b1, float b2, float eps,
                         float rescale, const void* skip_dev, void* stream) {
    if (!e || !table_host || ntensors < 1 || ntensors > 4096) return fail(APZ_E_ARG, "bad argument");
    static_assert(sizeof(apz::AdamTensor) == 48, "apz_adam_tensor layout");
    return train_call(e, stream, [&]() -> int {
        const apz::AdamTensor* tab;
        if (int rc = upload_table(e, e->adam_tab, table_host, ntensors, &tab)) return rc;
        if (skip_dev)      // (two kernels with two signatures)
            hipLaunchKernelGGL(apz::adam_step_unless_kernel, dim3(32, ntensors), dim3(256), 0, e->stream, tab, lr_t, b1, b2, eps,
                               rescale, (const unsigned*)skip_dev);
        else
            hipLaunchKernelGGL(apz::adam_step_kernel, dim3(32, ntensors), dim3(256), 0, e->stream, tab, lr_t, b1, b2, eps, rescale);
        return APZ_OK;
    });
}

// ---- the guarded optimiser step (csrc/grad_guard.h)
namespace {
bool guard_args_ok(const apz_engine* e, const void* table_host, int ntensors, const void* record_dev) {
    return e && table_host && ntensors >= 1 && ntensors <= 4096 && record_dev && ((uintptr_t)record_dev & 15) == 0;
}
// inside a train_call: the table uploaded, the two reduction launches queued
int queue_grad_guard(apz_engine* e, const void* table_host, int ntensors, float rescale, float clip, const void* loss3_dev,
                     const void* skip_in_dev, void* record_dev) {
    const size_t parts = (size_t)ntensors * apz::GUARD_SPLITS;
    if (int rc = e->guard_part.reserve(parts * (sizeof(double) + sizeof(unsigned)))) return rc;
    double* part = e->guard_part.as<double>();
    unsigned* bad = (unsigned*)(part + parts);
    const apz::AdamTensor* tab;
    if (int rc = upload_table(e, e->adam_tab, table_host, ntensors, &tab)) return rc;
    hipLaunchKernelGGL(apz::grad_sumsq_kernel, dim3(apz::GUARD_SPLITS, ntensors), dim3(256), 0, e->stream, tab, part, bad);
    hipLaunchKernelGGL(apz::grad_guard_fold_kernel, dim3(1), dim3(256), 0, e->stream, (const double*)part, (const unsigned*)bad,
                       ntensors, rescale, clip, (const float*)loss3_dev, (const unsigned*)skip_in_dev, (apz::GuardRecord*)record_dev);
    return APZ_OK;
}
}  // namespace

int apz_grad_norm(apz_engine* e, const void* table_host, int ntensors, float rescale, float clip, const void* loss3_dev,
                  const void* skip_in_dev, void* record_dev, void* stream) {
    if (!guard_args_ok(e, table_host, ntensors, record_dev)) return fail(APZ_E_ARG, "bad argument");
    static_assert(sizeof(apz::GuardRecord) == 16, "apz guard record layout");
    return train_call(e, stream, [&]() -> int {
        return queue_grad_guard(e, table_host, ntensors, rescale, clip, loss3_dev, skip_in_dev, record_dev);
    });
}

int apz_adam_step_guarded(apz_engine* e, const void* table_host, int ntensors, float lr_t, float b1, float b2, float eps,
                          float rescale, float clip, const void* loss3_dev, const void* skip_in_dev, void* record_dev,
                          void* stream) {
    if (!guard_args_ok(e, table_host, ntensors, record_dev)) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        if (int rc = queue_grad_guard(e, table_host, ntensors, rescale, clip, loss3_dev, skip_in_dev, record_dev)) return rc;
        hipLaunchKernelGGL(apz::adam_step_guarded_kernel, dim3(32, ntensors), dim3(256), 0, e->stream,
                           e->adam_tab.as<const apz::AdamTensor>(), lr_t, b1, b2, eps, (const apz::GuardRecord*)record_dev);
        return APZ_OK;
    });
}

// ---- the averaged weights (csrc/ema.h)
int apz_ema_update(apz_engine* e, const void* table_host, int ntensors, float c, const void* skip_a_dev, const void* skip_b_dev,
                   void* stream) {
    if (!e || ntensors < 0 || ntensors > 4096 || (ntensors > 0 && !table_host)) return fail(APZ_E_ARG, "bad argument");
    static_assert(sizeof(apz::EmaTensor) == 24, "apz_ema_tensor layout");
    if (ntensors == 0) return APZ_OK;       // an empty table: nothing to launch (a grid of (32, 0) is not one)
    return train_call(e, stream, [&]() -> int {
        // through Adam's device buffer: the copy queues behind the Adam launch in front of it, which read its own table there
        const apz::EmaTensor* tab;
        if (int rc = upload_table(e, e->adam_tab, table_host, ntensors, &tab)) return rc;
        hipLaunchKernelGGL(apz::ema_update_kernel, dim3(32, ntensors), dim3(256), 0, e->stream, tab, c,
                           (const unsigned*)skip_a_dev, (const unsigned*)skip_b_dev);
        return APZ_OK;
    });
}

// ---- heads and loss of the training graph (csrc/heads_train.h)
namespace {
// C[M][N] = A B (+ bias): 64 x 64 tiles per workgroup when those fill the chip, else 16 x 16 tiles with the k-steps split over the waves
void launch_sgemm(apz_engine* e, const float* a, const float* b, const float* bias, float* c, int M, int N, int K, long a_rs,
                  long a_cs, long b_rs, long b_cs, int ldc) {
    const int my = (M + 63) / 64;
    if (((N + 63) / 64) * my >= e->num_cu / 2)
        hipLaunchKernelGGL(apz::sgemm_mfma_kernel<4>, dim3((N + 63) / 64, my), dim3(256), 0, e->stream, a, b, bias, c, M, N, K, a_rs,
                           a_cs, b_rs, b_cs, ldc);
    else
        hipLaunchKernelGGL(apz::sgemm_ksplit_kernel, dim3((N + 15) / 16, (M + 15) / 16), dim3(256), 0, e->stream, a, b, bias, c, M,
                           N, K, a_rs, a_cs, b_rs, b_cs, ldc);
}
}  // namespace

namespace {
// the window a 1x1 head convolution walks: H x W cells in planes of `ps` floats, rows of `rs`
struct HeadGeo { int H, W, ps, rs; };
// frame null: the engine's board in `layout`; else the side x side window of a padded-row trunk tensor (framed boards;
// frame = the entry point's name for the refusal)
int head_geometry(apz_engine* e, int layout, int side, const char* frame, HeadGeo* g) {
    if (frame) {
        *g = {side, side, apz::Frame15::GPLANE, apz::Frame15::GROW};
        return frame_train_check(e, side, frame);
    }
    g->H = e->cfg.height, g->W = e->cfg.width;
    return bn_geometry(e, layout, &g->ps, &g->rs);
}

int conv1x1_fwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int n, int C, int CO,
                int layout, int side, const char* frame, void* stream) {
    if (!e || !x_dev || !w_dev || !y_dev || n < 1 || C < 1 || C > 1024 || CO < 1 || CO > 8) return fail(APZ_E_ARG, "bad argument");
    HeadGeo g;
    if (int rc = head_geometry(e, layout, side, frame, &g)) return rc;
    return train_call(e, stream, [&]() -> int {
        const int lds = (CO * C + 4 * 8 * 64) * (int)sizeof(float);
        if (int rc = need_lds(e, (const void*)apz::conv1x1_fwd_kernel, lds)) return rc;
        hipLaunchKernelGGL(apz::conv1x1_fwd_kernel, dim3(n, (g.H * g.W + 63) / 64), dim3(256), lds, e->stream, (const float*)x_dev,
                           (const float*)w_dev, (const float*)bias_dev, (float*)y_dev, C, CO, g.H, g.W, g.ps, g.rs);
        return APZ_OK;
    });
}

int conv1x1_bwd2(apz_engine* e, const void* x_dev, const void* w1_dev, const void* dy1_dev, int CO1, const void* w2_dev,
                 const void* dy2_dev, int CO2, void* dx_dev, void* dw_dev, int n, int C, int layout, int side, const char* frame,
                 int accumulate_dx, void* stream) {
    if (!e || !x_dev || !w1_dev || !dy1_dev || !dw_dev || n < 1 || C < 1 || C > 1024 || CO1 < 1 || CO2 < 0 || CO1 + CO2 > 8 ||
        (CO2 > 0 && (!w2_dev || !dy2_dev)))
        return fail(APZ_E_ARG, "bad argument");
    HeadGeo g;
    if (int rc = head_geometry(e, layout, side, frame, &g)) return rc;
    return train_call(e, stream, [&]() -> int {
        const int P = g.H * g.W, CO = CO1 + CO2;
        if (int rc = e->head_scratch.reserve((size_t)n * CO * C * sizeof(float))) return rc;
        float* part = e->head_scratch.as<float>();      // dw per board
        const int lds = (CO * 32 + CO * P) * (int)sizeof(float);
        if (int rc = need_lds(e, (const void*)apz::conv1x1_bwd_kernel, lds)) return rc;
        hipLaunchKernelGGL(apz::conv1x1_bwd_kernel, dim3(n, (C + 31) / 32), dim3(256), lds, e->stream, (const float*)x_dev,
                           (const float*)w1_dev, (const float*)dy1_dev, (const float*)w2_dev, (const float*)dy2_dev, (float*)dx_dev,
                           part, C, CO1, CO2, g.H, g.W, g.ps, g.rs, accumulate_dx);
        hipLaunchKernelGGL(apz::colsum_kernel, dim3((CO * C + 63) / 64), dim3(256), 0, e->stream, (const float*)part,
                           (float*)dw_dev, n, CO * C, 1.0f);
        return APZ_OK;
    });
}
}  // namespace

int apz_conv1x1_fwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int n, int C,
                    int CO, int layout, void* stream) {
    return conv1x1_fwd(e, x_dev, w_dev, bias_dev, y_dev, n, C, CO, layout, 0, nullptr, stream);
}

int apz_conv1x1_bwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* dy_dev, void* dx_dev, void* dw_dev,
                    void* db_dev, int n, int C, int CO, int layout, int accumulate_dx, void* stream) {
    if (int rc = apz_conv1x1_bwd2(e, x_dev, w_dev, dy_dev, CO, nullptr, nullptr, 0, dx_dev, dw_dev, n, C, layout, accumulate_dx, stream))
        return rc;
    if (db_dev) return apz_bias_grad(e, dy_dev, db_dev, n, CO, APZ_LAYOUT_DENSE, stream);
    return APZ_OK;
}

int apz_conv1x1_bwd2(apz_engine* e, const void* x_dev, const void* w1_dev, const void* dy1_dev, int CO1, const void* w2_dev,
                     const void* dy2_dev, int CO2, void* dx_dev, void* dw_dev, int n, int C, int layout, int accumulate_dx,
                     void* stream) {
    return conv1x1_bwd2(e, x_dev, w1_dev, dy1_dev, CO1, w2_dev, dy2_dev, CO2, dx_dev, dw_dev, n, C, layout, 0, nullptr,
                        accumulate_dx, stream);
}

// ... on the S x S window of a padded-row trunk tensor (framed boards): the same two kernels with H = W = side on planes of
// 240 floats in rows of 16.  Forward: y dense [n][CO][side][side].  Backward: dx rows 0 .. side - 1 are written (columns
// side .. 15 zero), rows side .. 14 are NOT -- apz_bn_bwd_frame, the consumer, selects them away.
int apz_conv1x1_fwd_frame(apz_engine* e, const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int n, int C,
                          int CO, int side, void* stream) {
    return conv1x1_fwd(e, x_dev, w_dev, bias_dev, y_dev, n, C, CO, APZ_LAYOUT_ROWS16, side, "conv1x1_fwd_frame", stream);
}

int apz_conv1x1_bwd2_frame(apz_engine* e, const void* x_dev, const void* w1_dev, const void* dy1_dev, int CO1, const void* w2_dev,
                           const void* dy2_dev, int CO2, void* dx_dev, void* dw_dev, int n, int C, int side, int accumulate_dx,
                           void* stream) {
    return conv1x1_bwd2(e, x_dev, w1_dev, dy1_dev, CO1, w2_dev, dy2_dev, CO2, dx_dev, dw_dev, n, C, APZ_LAYOUT_ROWS16, side,
                        "conv1x1_bwd2_frame", accumulate_dx, stream);
}

int apz_bias_grad(apz_engine* e, const void* dy_dev, void* db_dev, int n, int C, int layout, void* stream) {
    if (!e || !dy_dev || !db_dev || n < 1 || C < 1) return fail(APZ_E_ARG, "bad argument");
    int ps, rs;
    if (int rc = bn_geometry(e, layout, &ps, &rs)) return rc;
    return train_call(e, stream, [&]() -> int {
        const int slices = std::max(1, std::min(n, (e->num_cu * 8 + C - 1) / C));
        if (int rc = e->head_scratch.reserve((size_t)slices * C * sizeof(float))) return rc;
        float* part = e->head_scratch.as<float>();      // db per slice of the batch
        hipLaunchKernelGGL(apz::bias_grad_kernel, dim3(C, slices), dim3(256), 0, e->stream, (const float*)dy_dev, part, n, C, ps);
        hipLaunchKernelGGL(apz::colsum_kernel, dim3((C + 63) / 64), dim3(256), 0, e->stream, (const float*)part, (float*)db_dev,
                           slices, C, 1.0f);
        return APZ_OK;
    });
}

int apz_add(apz_engine* e, void* y_dev, const void* x_dev, int64_t count, void* stream) {
    if (!e || !y_dev || !x_dev || count < 1) return fail(APZ_E_ARG, "bad argument");
    if (((uintptr_t)y_dev | (uintptr_t)x_dev) & 15) return fail(APZ_E_ARG, "add: 16-byte aligned tensors");
    return train_call(e, stream, [&]() -> int {
        const long n4 = count / 4;
        hipLaunchKernelGGL(apz::add_inplace_kernel, dim3((int)std::max<long>(1, std::min<long>((n4 + 255) / 256, 8192))), dim3(256), 0,
                           e->stream, (float*)y_dev, (const float*)x_dev, n4, (long)count);
        return APZ_OK;
    });
}

int apz_fc_fwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int n, int K, int N,
               void* stream) {
    if (!e || !x_dev || !w_dev || !y_dev || n < 1 || K < 1 || N < 1) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        // y[n][N] = x[n][K] W[N][K]^T + b:  A = x (row stride K), B(k, j) = W[j][k]
        launch_sgemm(e, (const float*)x_dev, (const float*)w_dev, (const float*)bias_dev, (float*)y_dev, n, N, K, (long)K, 1L, 1L,
                     (long)K, N);
        return APZ_OK;
    });
}

int apz_fc_bwd(apz_engine* e, const void* x_dev, const void* w_dev, const void* dy_dev, void* dx_dev, void* dw_dev, void* db_dev,
               int n, int K, int N, void* stream) {
    if (!e || !x_dev || !w_dev || !dy_dev || n < 1 || K < 1 || N < 1) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        if (dx_dev)     // dx[n][K] = dy[n][N] W[N][K]
            launch_sgemm(e, (const float*)dy_dev, (const float*)w_dev, nullptr, (float*)dx_dev, n, K, N, (long)N, 1L, (long)K, 1L, K);
        if (dw_dev)     // dW[N][K] = dy^T[N][n] x[n][K]:  A(m, k) = dy[k][m]
            launch_sgemm(e, (const float*)dy_dev, (const float*)x_dev, nullptr, (float*)dw_dev, N, K, n, 1L, (long)N, (long)K, 1L, K);
        if (db_dev)
            hipLaunchKernelGGL(apz::colsum_kernel, dim3((N + 63) / 64), dim3(256), 0, e->stream, (const float*)dy_dev, (float*)db_dev,
                               n, N, 1.0f);
        return APZ_OK;
    });
}

int apz_dropout(apz_engine* e, const void* x_dev, void* y_dev, int64_t count, float keep, uint64_t seed, uint64_t step,
                void* stream) {
    if (!e || !x_dev || !y_dev || count < 1 || !(keep > 0.f) || keep > 1.f) return fail(APZ_E_ARG, "bad argument");
    return train_call(e, stream, [&]() -> int {
        hipLaunchKernelGGL(apz::dropout_kernel, dim3((int)std::min<int64_t>((count + 255) / 256, 4096)), dim3(256), 0, e->stream,
                           (const float*)x_dev, (float*)y_dev, (long)count, keep, (unsigned long long)seed, (unsigned long long)step);
        return APZ_OK;
    });
}

// apz_pv_loss (occ_dev == NULL) and apz_pv_loss_legal: the loss kernel of the form, then the batch means
static int pv_loss_call(apz_engine* e, const void* logits_dev, const void* vlogit_dev, const void* pi_dev, const void* z_dev,
                        const void* occ_dev, int n, void* loss3_dev, void* dlogits_dev, void* dvlogit_dev, void* probs_dev,
                        void* values_dev, void* stream) {
    if (!e || !logits_dev || !vlogit_dev || n < 1) return fail(APZ_E_ARG, "bad argument");
    if ((loss3_dev || dlogits_dev || dvlogit_dev) && (!pi_dev || !z_dev)) return fail(APZ_E_ARG, "targets missing");
    if (e->hw > 4096) return fail(APZ_E_UNSUPPORTED, "board too large");
    return train_call(e, stream, [&]() -> int {
        if (int rc = e->head_scratch.reserve((size_t)n * 3 * sizeof(float))) return rc;
        float* part = e->head_scratch.as<float>();      // the three terms per sample
        float* terms = loss3_dev ? part : (float*)nullptr;
        const dim3 grid((n + 3) / 4), block(256);
        hipLaunchKernelGGL(occ_dev ? apz::pv_loss_kernel<true> : apz::pv_loss_kernel<false>, grid, block, 0, e->stream,
                           (const float*)logits_dev, (const float*)vlogit_dev, (const float*)pi_dev, (const float*)z_dev,
                           (const unsigned char*)occ_dev, n, e->hw, 1.0f / (float)n, terms, (float*)dlogits_dev,
                           (float*)dvlogit_dev, (float*)probs_dev, (float*)values_dev);
        if (loss3_dev)  // (value loss, policy loss, entropy): batch means, samples summed in index order
            hipLaunchKernelGGL(apz::colsum_kernel, dim3(1), dim3(256), 0, e->stream, (const float*)part, (float*)loss3_dev, n, 3,
                               1.0f / (float)n);
        return APZ_OK;
    });
}

int apz_pv_loss(apz_engine* e, const void* logits_dev, const void* vlogit_dev, const void* pi_dev, const void* z_dev, int n,
                void* loss3_dev, void* dlogits_dev, void* dvlogit_dev, void* probs_dev, void* values_dev, void* stream) {
    return pv_loss_call(e, logits_dev, vlogit_dev, pi_dev, z_dev, nullptr, n, loss3_dev, dlogits_dev, dvlogit_dev, probs_dev,
                        values_dev, stream);
}

int apz_pv_loss_legal(apz_engine* e, const void* logits_dev, const void* vlogit_dev, const void* pi_dev, const void* z_dev,
                      const void* occ_dev, int n, void* loss3_dev, void* dlogits_dev, void* dvlogit_dev, void* probs_dev,
                      void* values_dev, void* stream) {
    if (!occ_dev) return fail(APZ_E_ARG, "bad argument");
    return pv_loss_call(e, logits_dev, vlogit_dev, pi_dev, z_dev, occ_dev, n, loss3_dev, dlogits_dev, dvlogit_dev, probs_dev,
                        values_dev, stream);
}

int apz_occupancy_planes(apz_engine* e, const void* planes_dev, int n, int c_in, int H, int W, void* occ_dev, void* stream) {
    if (!e || !planes_dev || !occ_dev) return fail(APZ_E_ARG, "null argument");
    if (c_in != 9 && c_in != 4) return fail(APZ_E_ARG, "occupancy: c_in must be 9 or 4");
    if (n < 0 || H < 1 || W < 1) return fail(APZ_E_ARG, "occupancy: bad batch / board");
    if (n == 0) return APZ_OK;
    return train_call(e, stream, [&]() -> int { return launch_occupancy_planes(e, (const float*)planes_dev, n, c_in, H, W, (unsigned char*)occ_dev); });
}

int apz_layout_convert(apz_engine* e, const void* src_dev, void* dst_dev, int64_t planes, int to_rows16, void* stream) {
    if (!e || !src_dev || !dst_dev || planes < 1) return fail(APZ_E_ARG, "bad argument");
    if (e->cfg.height != 15 || e->cfg.width != 15) return fail(APZ_E_UNSUPPORTED, "padded-row layout: 15x15 boards only");
    return train_call(e, stream, [&]() -> int {
        const int grid = (int)std::min<int64_t>((planes * 240 + 255) / 256, 16384);
        const auto kern = to_rows16 ? apz::rows16_from_dense_kernel : apz::rows16_to_dense_kernel;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, e->stream, (const float*)src_dev, (float*)dst_dev, (long)planes);
        return APZ_OK;
    });
}

// dense [planes][side][side] -> dense [planes][15][15], off-board cells zero (frame_planes_kernel of the framed evaluator)
int apz_frame_planes_dev(apz_engine* e, const void* src_dev, void* dst_dev, int64_t planes, int side, void* stream) {
    if (!e || !src_dev || !dst_dev || planes < 1) return fail(APZ_E_ARG, "bad argument");
    if (int rc = frame_train_check(e, side, "frame_planes_dev")) return rc;
    return train_call(e, stream, [&]() -> int {
        const long total = (long)planes * apz::Frame15::CELLS;
        hipLaunchKernelGGL(apz::frame_planes_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 8)), dim3(256), 0,
                           e->stream, (const float*)src_dev, (float*)dst_dev, (long)planes, side);
        return APZ_OK;
    });
}

// ---- device replay buffer (csrc/replay.h)
int apz_replay_gather(apz_engine* e, const void* codes_dev, const void* pi_dev, const void* z_dev, int64_t capacity,
                      const int32_t* entries_host, int n, int n_planes, void* planes_out_dev, void* pi_out_dev, void* z_out_dev,
                      void* stream) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    if (!e->perm_s) return fail(APZ_E_UNSUPPORTED, "the replay gather needs a square board");
    if (n_planes != 9 && n_planes != 4) return fail(APZ_E_ARG, "n_planes must be 9 or 4");
    if (n < 0 || capacity < 0 || capacity > (INT32_MAX >> 3)) return fail(APZ_E_ARG, "replay gather: bad sample count / capacity");
    if (n == 0) return APZ_OK;
    if (!codes_dev || !pi_dev || !z_dev || !entries_host || !planes_out_dev || !pi_out_dev || !z_out_dev)
        return fail(APZ_E_ARG, "null argument");
    // every entry before anything is copied or launched: the kernel indexes the ring with them unchecked
    for (int j = 0; j < n; j++)
        if (entries_host[j] < 0 || (int64_t)entries_host[j] >= 8 * capacity)
            return fail(APZ_E_ARG, "replay gather: entry " + std::to_string(j) + " = " + std::to_string(entries_host[j]) +
                                       " lies outside [0, 8 * capacity = " + std::to_string(8 * capacity) + ")");
    return train_call(e, stream, [&]() -> int {
        const int* entries;
        if (int rc = upload_table(e, e->gather_entries, entries_host, n, &entries)) return rc;
        const long total = (long)n * e->hw;
        hipLaunchKernelGGL(apz::replay_gather_kernel, dim3((int)std::min<long>((total + 255) / 256, e->num_cu * 16)), dim3(256), 0,
                           e->stream, (const unsigned char*)codes_dev, (const float*)pi_dev, (const float*)z_dev,
                           entries, e->perm_s, e->perm_p, (float*)planes_out_dev, (float*)pi_out_dev,
                           (float*)z_out_dev, n, e->cfg.height, e->cfg.width, e->code_stride, n_planes);
        return APZ_OK;
    });
}

// apz_forward_host for planes that already live in device memory (a mini-batch of the device replay buffer): the engine's
// stream waits for what `after_stream` has queued so far (the kernel that wrote the planes), runs the same forward and
// copies the results out.  Returns with the engine's stream drained: the planes may be released or rewritten.
int apz_forward_dev_host(apz_engine* e, const void* planes_dev, int n, float* probs_host, float* values_host, void* after_stream) {
    if (!e || !planes_dev || !probs_host || !values_host) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (n < 0 || n > e->cfg.max_batch) return fail(APZ_E_ARG, "batch exceeds max_batch");
    if (n == 0) return APZ_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (after_stream != APZ_ENGINE_STREAM && (hipStream_t)after_stream != e->stream)
        HIP_TRY(stream_wait(e, e->stream, (hipStream_t)after_stream));
    return forward_to_host(e, n, [&](const FwdMode& m) {
        return forward_dev(e, m, (const float*)planes_dev, nullptr, n, e->probs, e->values);
    }, probs_host, values_host);
}

int apz_prewarm(apz_engine* e, int n, int iters) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    if (n < 1 || n > e->cfg.max_batch || iters < 0) return fail(APZ_E_ARG, "prewarm: bad batch / iteration count");
    EngineLock guard(e->submit_lock);
    if (!e->loaded) return fail(APZ_E_STATE, "weights not loaded");
    HIP_TRY(hipSetDevice(e->cfg.device));
    // e->codes is zero-filled at creation and only ever overwritten with valid codes: any content is a legal input
    const FwdMode m = armed(e, APZ_MAX_SLOTS);   // (raised, and nobody reads it)
    for (int i = 0; i < iters; i++)
        if (int rc = forward_from_codes(e, m, e->codes, n, e->probs, e->values)) return rc;
    return APZ_OK;
}

int apz_sync(apz_engine* e) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    resolve_pending(e);
    return APZ_OK;
}

void* apz_stream(apz_engine* e) { return e ? (void*)e->stream : nullptr; }

void* apz_device_alloc(apz_engine* e, int64_t bytes) {
    void* p = nullptr;
    if (!e || bytes <= 0 || hipSetDevice(e->cfg.device) != hipSuccess || hipMalloc(&p, (size_t)bytes) != hipSuccess) {
        fail(APZ_E_HIP, "hipMalloc failed");
        return nullptr;
    }
    return p;
}

void apz_device_free(apz_engine* e, void* p) {
    if (e && p) {
        hipSetDevice(e->cfg.device);
        hipFree(p);
    }
}

int apz_memcpy_h2d(apz_engine* e, void* dst_dev, const void* src_host, int64_t bytes) {
    if (!e || !dst_dev || !src_host || bytes < 0) return fail(APZ_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return APZ_OK;
}

int apz_memcpy_d2h(apz_engine* e, void* dst_host, const void* src_dev, int64_t bytes) {
    if (!e || !dst_host || !src_dev || bytes < 0) return fail(APZ_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return APZ_OK;
}

int apz_conv3x3_bench(apz_engine* e, int layer, int n, int iters, int warmup, float* ms_out) {
    if (!e || !ms_out) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (!e->loaded) return fail(APZ_E_STATE, "weights not loaded");
    if (layer < 0 || layer >= (int)e->convs.size() || n < 1 || n > e->cfg.max_batch || iters < 1 || warmup < 0)
        return fail(APZ_E_ARG, "bad layer / batch / iteration count");
    HIP_TRY(hipSetDevice(e->cfg.device));
    FwdMode m = armed(e, APZ_MAX_SLOTS);          // (raised, and nobody reads it)
    m.untimed = true;
    // produce this layer's real input from the planes resident in e->planes
    const float* in = e->planes;
    if (layer > 0) {
        float* prev = nullptr;
        if (int rc = run_trunk(e, m, e->planes, nullptr, n, layer - 1, &prev)) return rc;
        in = prev;
    }
    const ConvLayer& L = e->convs[layer];
    float* out = nullptr;
    const float* resid = nullptr;
    for (int i = 0; i < 3; i++)
        if (e->act[i] != in && !out) out = e->act[i];
    if (L.residual)
        for (int i = 0; i < 3; i++)
            if (e->act[i] != in && e->act[i] != out) resid = e->act[i];
    auto launch = [&]() { return layer > 0 ? launch_conv(e, m, L, in, resid, out, n) : launch_first_layer(e, m, in, nullptr, out, n); };
    hipEvent_t a = get_event(e), b = get_event(e);   // pooled, destroyed with the engine
    int rc = APZ_OK;
    for (int i = 0; i < warmup && !rc; i++) rc = launch();
    hipError_t he = hipEventRecord(a, e->stream);
    for (int i = 0; i < iters && !rc; i++) rc = launch();
    if (he == hipSuccess) he = hipEventRecord(b, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, a, b);
    e->free_events.push_back(a);
    e->free_events.push_back(b);
    if (he != hipSuccess) return fail(APZ_E_HIP, std::string("conv bench timing: ") + hipGetErrorString(he));
    if (rc) return rc;
    ms_out[0] = ms / iters;
    return APZ_OK;
}

namespace {
// apz_layer_io / apz_layer_frame: the trunk of the last forward's batch again on the planes resident in e->planes, up to
// `layer`, whose output of `count` = n*C_out*plane floats is then in *buf
int rerun_to_layer(apz_engine* e, int layer, int64_t count, int plane, const char* plane_name, float** buf) {
    if (!e->loaded || e->last_n < 1) return fail(APZ_E_STATE, "run a forward first");
    if (layer < 0 || layer >= (int)e->convs.size()) return fail(APZ_E_ARG, "bad layer");
    const int64_t need = (int64_t)e->last_n * e->convs[layer].cout * plane;
    if (count != need) return fail(APZ_E_ARG, std::string("count must be n*C_out*") + plane_name + " = " + std::to_string(need));
    HIP_TRY(hipSetDevice(e->cfg.device));
    FwdMode m = armed(e, APZ_MAX_SLOTS);          // (raised, and nobody reads it)
    m.untimed = true;
    return run_trunk(e, m, e->planes, nullptr, e->last_n, layer, buf);
}
}  // namespace

int apz_layer_io(apz_engine* e, int layer, float* host_out, int64_t count) {
    if (!e || !host_out) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    float* buf = nullptr;
    if (int rc = rerun_to_layer(e, layer, count, e->hw, "H*W", &buf)) return rc;
    if (!e->ring) {
        HIP_TRY(hipMemcpyAsync(host_out, buf, count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return APZ_OK;
    }
    const int C = e->convs[layer].cout, H = e->cfg.height, W = e->cfg.width;
    std::vector<float> tmp((size_t)e->last_n * C * e->act_ps);
    HIP_TRY(hipMemcpyAsync(tmp.data(), buf, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t pc = 0; pc < (size_t)e->last_n * C; pc++)
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) host_out[(pc * H + y) * W + x] = tmp[pc * e->act_ps + y * e->act_rs + x];
    return APZ_OK;
}

int apz_layer_frame(apz_engine* e, int layer, float* host_out, int64_t count) {
    if (!e || !host_out) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (!e->ring) return fail(APZ_E_UNSUPPORTED, "layer_frame: engines with rows16 activations only (the 128-filter residual net at 15x15 and at framed sizes)");
    float* buf = nullptr;
    if (int rc = rerun_to_layer(e, layer, count, e->act_ps, "15*16", &buf)) return rc;
    HIP_TRY(hipMemcpyAsync(host_out, buf, count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return APZ_OK;
}

int apz_set_trunk_arith(apz_engine* e, int arith) {
    if (e) {
        EngineLock guard_(e->submit_lock);
        drop_forward_graphs(e);
    }
    if (!e || (arith != APZ_ARITH_F32 && arith != APZ_ARITH_BF16X3 && arith != APZ_ARITH_F16X2))
        return fail(APZ_E_ARG, "bad trunk arithmetic");
    EngineLock guard(e->submit_lock);
    if (arith == APZ_ARITH_BF16X3 && !e->ring)
        return fail(APZ_E_UNSUPPORTED, "the bf16 x 3 trunk kernel exists for the 15x15 / 128-filter residual net only");
    if (arith == APZ_ARITH_F16X2 && !e->ring && !e->small8 && !(e->cfg.height == 15 && e->cfg.width == 15))
        return fail(APZ_E_UNSUPPORTED, "the fp16 x 2 split kernels exist for 15x15 boards, for the 128-filter residual net on the boards framed in them and for 8x8 boards");
    if (arith == APZ_ARITH_F16X2 && !e->ovf_host) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(hipHostMalloc((void**)&e->ovf_host, (APZ_MAX_SLOTS + 1) * sizeof(unsigned), hipHostMallocMapped));
        std::memset(e->ovf_host, 0, (APZ_MAX_SLOTS + 1) * sizeof(unsigned));
        HIP_TRY(hipHostGetDevicePointer((void**)&e->ovf_dev, e->ovf_host, 0));
    }
    if (e->loaded && arith != e->trunk_arith)
        return fail(APZ_E_STATE, "apz_set_trunk_arith must be called before the weights are loaded");
    e->trunk_arith = arith;
    return APZ_OK;
}

long apz_trunk_overflows(apz_engine* e) { return e ? e->ovf_repeats : -1; }

int apz_set_trunk_act_exponents(apz_engine* e, const int* a, int count) {
    if (!e || !a) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (int rc = act_scale_supported(e)) return rc;
    if (!e->loaded) return fail(APZ_E_STATE, "weights not loaded");
    const int layers = (int)e->convs.size() - 1;
    if (count != layers) return fail(APZ_E_ARG, "activation exponents: count must be 2 * n_blocks = " + std::to_string(layers));
    for (int l = 0; l < count; l++)
        if (a[l] < -apz::ACT_EXP_MAX || a[l] > apz::ACT_EXP_MAX)
            return fail(APZ_E_ARG, "activation exponents must lie in [-100, 100]");
    HIP_TRY(hipSetDevice(e->cfg.device));
    std::vector<int> eff(count);
    for (int l = 0; l < count; l++)
        if (int rc = clamp_act_exponent(e, e->convs[l + 1], a[l], &eff[l])) return rc;
    drop_forward_graphs(e);                       // a captured launch sequence holds the old exponents
    for (int l = 0; l < count; l++) e->convs[l + 1].act_exp = eff[l];
    return APZ_OK;
}

int apz_get_trunk_act_exponents(apz_engine* e, int* a, int count) {
    if (!e || !a) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    if (int rc = act_scale_supported(e)) return rc;
    const int layers = (int)e->convs.size() - 1;
    if (count != layers) return fail(APZ_E_ARG, "activation exponents: count must be 2 * n_blocks = " + std::to_string(layers));
    for (int l = 0; l < count; l++) a[l] = e->convs[l + 1].act_exp;
    return APZ_OK;
}

int apz_set_act_scale_auto(apz_engine* e, int on) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    if (int rc = act_scale_supported(e)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (on)
        if (int rc = act_scale_buffers(e)) return rc;
    e->act_auto = on != 0;
    return APZ_OK;
}

int apz_calibrate_trunk_planes(apz_engine* e, const float* planes_host, int n, float* layer_max_out, int count) {
    if (!e || !planes_host) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    return calibrate_trunk(e, n, layer_max_out, count, [&](const FwdMode& m) -> int {
        if (int rc = stage_planes(e, planes_host, n)) return rc;
        return forward_dev(e, m, e->planes, nullptr, n, e->probs, e->values);
    });
}

int apz_calibrate_trunk_codes(apz_engine* e, const uint8_t* codes_host, int n, float* layer_max_out, int count) {
    if (!e || !codes_host) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    return calibrate_trunk(e, n, layer_max_out, count, [&](const FwdMode& m) -> int {
        if (int rc = stage_codes(e, codes_host, n)) return rc;
        return forward_from_codes(e, m, e->codes, n, e->probs, e->values);
    });
}

int apz_test_select_trunk(apz_engine* e, int kind) {
    if (e) {
        EngineLock guard_(e->submit_lock);
        drop_forward_graphs(e);
    }
    if (!e || (kind != APZ_TRUNK_WINOGRAD && kind != APZ_TRUNK_DIRECT && kind != APZ_TRUNK_WINOGRAD_BATCHED &&
               kind != APZ_TRUNK_WINOGRAD_NO_QUARTER))
        return fail(APZ_E_ARG, "bad trunk kernel kind");
    EngineLock guard(e->submit_lock);
    if (!e->ring) return fail(APZ_E_UNSUPPORTED, "only the 15x15 / 128-filter residual net has two trunk kernels");
    e->trunk_kernel = kind == APZ_TRUNK_DIRECT ? APZ_TRUNK_DIRECT : APZ_TRUNK_WINOGRAD;
    e->no_small_trunk = kind == APZ_TRUNK_WINOGRAD_BATCHED || kind == APZ_TRUNK_WINOGRAD_NO_QUARTER;
    e->no_quarter_trunk = kind == APZ_TRUNK_WINOGRAD_NO_QUARTER;
    return APZ_OK;
}

int apz_set_trunk_uniform(apz_engine* e, int on) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    if (e->trunk_arith == APZ_ARITH_F32 || e->small8 || !e->ring) return APZ_OK;   // already uniform: one kernel family for every batch
    if (e->trunk_arith == APZ_ARITH_BF16X3)
        return fail(APZ_E_UNSUPPORTED, "the bf16 x 3 trunk kernel has no small-batch form: batches of <= 32 boards run exact fp32");
    if (e->f16x2_k8)
        return fail(APZ_E_UNSUPPORTED, "the 8-channel f16x2 kernel (APZ_F16X2_K8=1) has no small-batch form");
    if ((on != 0) != e->uniform_trunk) {
        drop_forward_graphs(e);                   // a captured launch sequence holds the other kernels ...
        e->fwd_seen.clear();                      // ... and the next capture waits until this route's lazy set-up has happened
    }
    e->uniform_trunk = on != 0;
    return APZ_OK;
}

int apz_set_leaf_symmetry(apz_engine* e, int mode, uint64_t seed) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    if (mode != APZ_SYM_NONE && mode != APZ_SYM_KEYED && mode != APZ_SYM_MEAN8)
        return fail(APZ_E_ARG, "leaf symmetry mode must be APZ_SYM_NONE (0), APZ_SYM_KEYED (1) or APZ_SYM_MEAN8 (2), not " +
                                   std::to_string(mode));
    EngineLock guard(e->submit_lock);
    if (!e->perm_p || e->cfg.height != e->cfg.width) return fail(APZ_E_UNSUPPORTED, "leaf symmetry needs a square board");
    if (e->code_stride > apz::LeafSym::MAX_STRIDE || e->code_stride % 16)     // (sym_expand_kernel's LDS row, its 16-byte loads)
        return fail(APZ_E_UNSUPPORTED, "leaf symmetry: the code row does not fit the expand kernel");
    for (const auto& sl : e->slots)
        if (sl.busy) return fail(APZ_E_STATE, "leaf symmetry: a slot is still in flight: call apz_wait first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (mode != APZ_SYM_NONE && !e->perm_pinv) {
        std::vector<int> ps, pp;
        build_perms(e->cfg.height, ps, pp);
        std::vector<int> inv(pp.size());
        for (int k = 0; k < 8; k++)
            for (int p = 0; p < e->hw; p++) inv[(size_t)k * e->hw + pp[(size_t)k * e->hw + p]] = p;
        if (int rc = upload(&e->perm_pinv, inv)) return rc;
    }
    drop_forward_graphs(e);                       // a captured launch sequence holds the other mode's launches and the old seed
    e->sym_mode = mode;
    e->sym_seed = seed;
    return APZ_OK;
}

int apz_set_legal_policy(apz_engine* e, int on) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    for (const auto& sl : e->slots)
        if (sl.busy) return fail(APZ_E_STATE, "legal policy: a slot is still in flight: call apz_wait first");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (on && !e->occ) HIP_TRY(hipMalloc((void**)&e->occ, (size_t)e->cfg.max_batch * e->hw));
    if ((on != 0) != e->legal_policy) drop_forward_graphs(e);      // a captured launch sequence holds the other heads
    e->legal_policy = on != 0;
    return APZ_OK;
}

int apz_get_legal_policy(apz_engine* e) { return e ? (int)e->legal_policy : fail(APZ_E_ARG, "null engine"); }

int apz_get_leaf_symmetry(apz_engine* e, int* mode, uint64_t* seed) {
    if (!e || !mode || !seed) return fail(APZ_E_ARG, "null argument");
    EngineLock guard(e->submit_lock);
    *mode = e->sym_mode;
    *seed = e->sym_seed;
    return APZ_OK;
}

int apz_leaf_symmetry_keys(const uint8_t* codes_host, int n, int hw, int stride, uint64_t seed, uint8_t* k_out) {
    if (n < 0 || hw < 1 || stride <= hw) return fail(APZ_E_ARG, "leaf symmetry keys: need n >= 0, hw >= 1 and stride > hw");
    if (n > 0 && (!codes_host || !k_out)) return fail(APZ_E_ARG, "null argument");
    for (int b = 0; b < n; b++)
        k_out[b] = (uint8_t)apz::leaf_sym_key(seed, codes_host + (size_t)b * stride, hw, 0, 1, [](uint64_t sum) { return sum; });
    return APZ_OK;
}

int apz_set_forward_graphs(apz_engine* e, int on) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    e->use_graphs = on != 0;
    if (!on) drop_forward_graphs(e);
    return APZ_OK;
}

int apz_set_profiling(apz_engine* e, int on) {
    if (!e) return fail(APZ_E_ARG, "null engine");
    EngineLock guard(e->submit_lock);
    HIP_TRY(hipStreamSynchronize(e->stream));
    resolve_pending(e);
    e->profiling = on != 0;
    e->prof_stride = on > 1 ? on : 1;   // on = k > 1: sample every k-th forward
    e->prof_phase = 0;
    for (int i = 0; i < APZ_K_COUNT; i++) {
        e->k_ms[i] = 0;
        e->k_cnt[i] = 0;
    }
    return APZ_OK;
}

int apz_kernel_time_ms(apz_engine* e, int kernel_class, float* out2) {
    if (!e || !out2 || kernel_class < 0 || kernel_class >= APZ_K_COUNT) return fail(APZ_E_ARG, "bad argument");
    EngineLock guard(e->submit_lock);
    out2[0] = (float)e->k_ms[kernel_class];
    out2[1] = (float)e->k_cnt[kernel_class];
    return APZ_OK;
}

}  // extern "C"
