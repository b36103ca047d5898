// Engine internals shared by engine.hip (Phi-3.5-V, LLaVA-1.6) and qwen.hip (Qwen2.5-VL): the weight-slot table,
// the handle and small host helpers.  Not part of the ABI (include/llava_reward_hip.h is).
#pragma once
#include "../../include/llava_reward_hip.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

using namespace lr;

inline thread_local std::string g_create_error;

inline uint64_t fnv1a64(const char* s) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (; *s; ++s) { h ^= (unsigned char)*s; h *= 0x100000001B3ull; }
    return h;
}
inline uint64_t splitmix64_host(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t tensor_seed(uint64_t seed, const char* name) { return splitmix64_host(seed ^ fnv1a64(name)); }
inline float uniform_scale(double std) { return (float)(std * std::sqrt(12.0) / 16777216.0); }

// One operand-typed weight buffer (oalloc) with everything the engine knows about it.  The GEMM kernels see raw pointers
// (Linear::params); the host passes the record around.
struct Weight {
    char* hi = nullptr; char* lo = nullptr;    // lo: the residual twin, null on handles created without split operands
    size_t bytes = 0;
    int id = 0;                // allocation order: lr_engine::inexact_dev[id]
    bool inexact = false;      // host copy of that flag (lr_engine::read_back_inexact): some 16-bit residual is non-zero
    // e4m3 twin of the residual pass.  Its rows live IN_LO: in the rows of lo (weights exact in the operand type: their
    // 16-bit residuals are all zero); OWN: in buf, a buffer the record keeps for good (adapter A matrices: the 16-bit residuals stay in
    // lo); PAIR: in buf as [e4m3(W) | e4m3(W_lo)] rows (inexact weights: the 16-bit residuals stay in lo, so the handle can still run
    // the strict form), allocated at the first preparation and given back once the weight is exact again.
    enum : int { IN_LO = 0, OWN = 1, PAIR = 2 };
    struct Lo8 { int where = IN_LO; void* buf = nullptr; int E = 127, E2 = 127; bool ready = false; } lo8;      // E, E2: E8M0 exponents of e4m3(W), e4m3(W_lo)
    const void* lo8_rows() const { return lo8.where == IN_LO ? lo : lo8.buf; }
    struct W8 { void* q = nullptr; float* scale = nullptr; bool ready = false; } w8;      // W8A8 twin (prepared on first use)
};

struct Slot {
    std::string name;
    std::vector<int64_t> shape;
    int rows, cols;            // 2-D view: [shape[0], prod(rest)] (1-D: [1, n])
    void* dst;                 // destination (already offset for concatenated tensors)
    int ld_dst, cols_dst, dst_dtype, mode;
    double std_, offset;       // synthetic init (llava_reward_amd.synth.weight_specs)
    int aux_d = 0, aux_hd = 0, aux_hdp = 0; // PACK_ROPE_QKV: rows of a section, head width, stored head width
    void* lo_dst = nullptr;    // split-operand mode: where the rounding residual of this tensor goes (same layout as dst)
    Weight* weight = nullptr;  // the operand-weight buffer that holds dst
    bool provided = false;
};

struct ClipLayer {
    Weight *qkv_w, *out_w, *fc1_w, *fc2_w;
    float *qkv_b, *out_b, *fc1_b, *fc2_b, *ln1_w, *ln1_b, *ln2_w, *ln2_b;
};
// Un-merged LoRA adapter of one (fused) linear y = x W^T (peft 0.13.2 tuners/lora/layer.py Linear.forward: result + lora_B(lora_A(x)) *
// scaling; the reference loads the adapter un-merged, eval/reward_adaptor_loader.py:44-45): t = x A^T is a GEMM of its own and
// y += t B^T rides in the K loop of the main GEMM as k2 extra columns (GemmParams::A2 / W2).  The scaling alpha / r is folded
// into B at upload.  A fused linear whose parts carry separate adapters (q/k/v, gate/up) stacks their A matrices (k2 = parts x
// padded rank) and holds B block-diagonally.
struct Lora {
    Weight* A = nullptr;       // [k2, K] operand dtype
    Weight* B = nullptr;       // [N, k2] operand dtype, rows packed like the base weight's
    int k2 = 0;                // 0 = no adapter
};
struct DecLayer {
    Weight *qkv_w, *o_w, *gu_w, *down_w;
    float *ln1, *ln2;
    float* qkv_b = nullptr;    // Qwen2.5-VL: q/k/v bias, packed like the rows of qkv_w
    Lora lqkv, lo, lgu, ldown;
};
struct VitLayer {              // Qwen2_5_VLVisionBlock
    Weight *qkv_w, *proj_w, *gu_w, *down_w;
    float *qkv_b, *proj_b, *gu_b, *down_b, *n1, *n2;
};

// Operand form of a stage or site: prec = split operands ([hi | lo] buffers, twice as wide), lo8 = ... with the residual pass of the
// big GEMMs in e4m3 (desc.precise == 2).  Passed to the producer and the consumer launched for a site; never a state.
struct Form { int prec, lo8; };

struct lr_engine {
    lr_model_desc d;
    int device = 0;
    std::string err;
    bool finalized = false;
    std::vector<void*> allocs;
    std::vector<Slot> slots;
    std::unordered_map<std::string, int> index;
    std::deque<Weight> weights;        // every operand-typed weight buffer, in allocation order (oalloc); addresses are stable
    // split-operand mode: every such buffer has a residual twin; a buffer is "inexact" once any residual is non-zero (launch_pack sets its word)
    int* inexact_dev = nullptr;
    size_t ws_bytes = 0;
    int gemm_tile = -1, lim_clip = -1, lim_layers = -1;
    uint64_t weights_epoch = 0;        // lr_weights_epoch: bumped by every call that changes a weight

    // derived
    int T = 0, G = 0, Kpatch = 0, Kpad = 0, hd = 0, half = 0, Vcap = 0;
    int Hq = 0, Hkv = 0, Nqkv = 0;      // decoder projection widths: heads*hd, kv_heads*hd, Hq + 2*Hkv
    bool llava = false, qwen = false;
    int op_dt = DT_BF16;
    Form created{0, 0};        // the form the handle was created with (desc.precise): sizes every buffer; written by lr_create only
    // block scales of one-byte residuals (common.h lo8_scale_at): two arrays used in turn -- a GEMM reads its operand's scales from
    // one while its epilogue writes its output's into the other -- and the row exponents of the e4m3 copy of a hi half
    unsigned char* sc[2] = {nullptr, nullptr}; size_t sc_cap = 0; int sc_i = 0;
    int* aexp2 = nullptr; size_t aexp2_cap = 0;
    unsigned* amax_word = nullptr;
    void* w8tmp = nullptr; size_t w8tmp_cap = 0;     // scratch of prepare_weight_e4m3_pair (Weight::PAIR twins)
    int lora_rp = 0, lora_k2max = 0;                 // adapter rank padded to a K-tile (64); widest K-extension of any linear
    void* lt = nullptr;                              // t = x A^T of the linear being launched, [rows, k2 (x2 in split-operand mode)]
    int w8a8 = 0;              // W8A8 mode (desc.w8a8): e4m3 GEMM operands with per-row / per-channel fp32 scales
    void* q8 = nullptr; size_t q8_cap = 0;           // quantised rows of the A operand of the GEMM being launched
    float* q8s = nullptr; size_t q8s_cap = 0;

    // Qwen2.5-VL ViT geometry: head dim vhd stored vhdp wide, MLP width vI stored vIp wide, patch vector vK padded to vKpad
    int vH = 0, vhd = 0, vhdp = 0, vHp = 0, vI = 0, vIp = 0, vK = 0, vKpad = 0, vHm = 0, vunit = 0;
    std::vector<VitLayer> vl;
    Weight *vpatch_w = nullptr, *m0_w = nullptr, *m2_w = nullptr;
    float *vlnq = nullptr, *m0_b = nullptr, *m2_b = nullptr, *vinv = nullptr, *ca_u = nullptr;
    void *vA = nullptr, *vhn = nullptr, *vqkv = nullptr, *vatt = nullptr, *vff = nullptr, *vm1 = nullptr;
    float *vx = nullptr, *vqkv32 = nullptr, *vcs = nullptr;
    int *pos3 = nullptr, *rstat = nullptr;
    int lastP = 0;

    // weights
    float *cls = nullptr, *pos = nullptr, *pre_w = nullptr, *pre_b = nullptr;
    Weight* patch_w = nullptr;
    std::vector<ClipLayer> cl;
    float *sub_gn = nullptr, *glb_gn = nullptr, *p0_b = nullptr, *p2_b = nullptr, *newline = nullptr;
    Weight *p0_w = nullptr, *p2_w = nullptr;
    unsigned short* wte = nullptr;
    std::vector<DecLayer> dl;
    float* norm_w = nullptr;
    float *Wq = nullptr, *WkT = nullptr, *Wv = nullptr;      // SkipCA projections for the fp32 tail, kept in fp32
    float *ca_w = nullptr, *vh = nullptr;
    float *inv_s = nullptr, *inv_l = nullptr;

    // staging for uploads
    void* stage_raw = nullptr; size_t stage_raw_cap = 0;
    float* stage_f32 = nullptr; size_t stage_f32_cap = 0;

    // workspace
    void *patchA = nullptr, *clip_h = nullptr, *clip_qkv = nullptr, *clip_att = nullptr, *clip_ff = nullptr;
    float *patch_out = nullptr, *clip_x = nullptr;
    void *hdA = nullptr, *proj1 = nullptr;
    float *ev = nullptr, *pf32 = nullptr;
    float *x = nullptr, *qkv32 = nullptr, *cs = nullptr;
    void *h = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr;
    int *pos_ids = nullptr, *img_row = nullptr, *tstat = nullptr;
    float *mh_h = nullptr, *mh_t1 = nullptr, *mh_t2 = nullptr, *mh_sc = nullptr;   // mean-pooling head (fp32, all tokens)
    float *hL = nullptr, *tq = nullptr, *tkq = nullptr, *tsc = nullptr, *tctx = nullptr, *tao = nullptr;
    // per-forward tables (ring of pinned host slots + device mirrors)
    static constexpr int NSLOT = 4;
    int slot_i = 0;
    char* tab_host = nullptr; char* tab_dev = nullptr; size_t tab_bytes = 0;
    hipEvent_t tab_ev[NSLOT] = {}; bool tab_used[NSLOT] = {};
    // last forward geometry (for taps)
    int lastB = 0, lastS = 0, lastNC = 0, lastSV = 0, lastVmax = 0;
    std::vector<int> last_voff;                      // first row in ev of every sample of the last forward (+ the end), lr_vision_embeds
    bool last_pruned = false;                        // the last forward ran its final decoder layer for the gathered rows only (x is stale there)
    // last decoder layer, gathered rows only (run_decoder_stack): compact [max_batch (+ pad), ...] twins of x / h / att / ff
    float* xg = nullptr; void *hg = nullptr, *attg = nullptr, *ffg = nullptr;
    int* sched_mem = nullptr;                        // tile-scheduler words of this engine's persistent GEMM launches (GemmParams::sched_mem)
    // precision map (lr_set_precision_map): operand form per stage, -1 = the descriptor's.  0 single pass, 1 split (16-bit residuals),
    // 2 split with e4m3 residual passes.  Decoder layers [pm_first, layers - pm_last) take pm_mid, the others the descriptor's form.
    int pm_clip = -1, pm_mid = -1, pm_first = 0, pm_last = 0;
    // ... and per SITE of a decoder layer in that range (lr_set_precision_sites, round 6): -1 = the layer's form.  A site = an operand
    // producer together with the GEMM (or attention launch) that reads it, so a site's form never crosses into its neighbours'.
    enum : int { SITE_QKV = 0, SITE_ATTN = 1, SITE_O = 2, SITE_GATE_UP = 3, SITE_DOWN = 4, N_SITES = 5 };
    int pm_site[N_SITES] = {-1, -1, -1, -1, -1};
    // lazy reference maximum of the attention launches in DEFAULT-form stages (lr_set_attention_lazy_threshold; log2 units, 0 = exact).
    // Strict stages run the exact maximum (att_lazy_t_strict = 0) except in the probe's noise-floor pass (model.py _compare_forms).
    float att_lazy_t = ATT_LAZY_T_DEFAULT, att_lazy_t_strict = 0.f;
    Form form(int m) const { return m < 0 ? created : Form{m ? 1 : 0, m == 2 ? 1 : 0}; }
    int layer_form(int l) const { return (pm_mid >= 0 && l >= pm_first && l < d.layers - pm_last) ? pm_mid : -1; }
    int site_form(int l, int site) const { const int f = layer_form(l); return (f >= 0 && pm_site[site] >= 0) ? pm_site[site] : f; }
    Form site(int l, int s) const { return form(site_form(l, s)); }
    // lr_set_layer_limits: how many decoder layers / layers of a `depth`-layer vision tower a pass runs
    int n_layers() const { return lim_layers >= 0 && lim_layers < d.layers ? lim_layers : d.layers; }
    int n_tower_layers(int depth) const { return lim_clip >= 0 && lim_clip < depth ? lim_clip : depth; }

    void* dalloc(size_t bytes, bool weight) {
        void* p = nullptr;
        bytes = (bytes + 255) & ~(size_t)255;
        LR_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 256));
        if (weight) LR_HIP_CHECK(hipMemset(p, 0, bytes ? bytes : 256));     // padded operand layouts rely on zero fill
        allocs.push_back(p);
        if (!weight) ws_bytes += bytes;
        return p;
    }
    // gives a dalloc'ed buffer back (ws_bytes: what it counted there)
    void dfree(void* p, size_t ws_counted = 0) {
        allocs.erase(std::find(allocs.begin(), allocs.end(), p));
        LR_HIP_CHECK(hipFree(p));
        ws_bytes -= (ws_counted + 255) & ~(size_t)255;
    }
    // Host copies of the inexact flags, behind a device synchronisation.  A weight that is exact in the operand type AGAIN (a re-upload /
    // re-synthesis replaced merged-adapter or fp32-valued weights) gives its PAIR rows (+1x its bytes) back: nothing reads them any more.
    void read_back_inexact() {
        if (!inexact_dev) return;
        std::vector<int> flags(weights.size());
        LR_HIP_CHECK(hipMemcpy(flags.data(), inexact_dev, flags.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (Weight& w : weights) {
            w.inexact = flags[w.id] != 0;
            if (w.inexact || w.lo8.where != Weight::PAIR) continue;
            dfree(w.lo8.buf);
            w.lo8 = Weight::Lo8{};
        }
    }
    // The bytes [dst, dst + bytes) of w are about to be rewritten (upload, re-synthesis): its twins are stale.
    void weight_changed(Weight& w, const void* dst, size_t bytes) {
        const bool whole = dst == w.hi && bytes == w.bytes;
        w.w8.ready = false;
        // an IN_LO twin overwrote the (all-zero) 16-bit residuals; the rows that this write leaves alone need theirs back
        if (w.lo8.ready && w.lo8.where == Weight::IN_LO && !whole) LR_HIP_CHECK(hipMemset(w.lo, 0, w.bytes));
        w.lo8.ready = false;
        if (whole && inexact_dev) LR_HIP_CHECK(hipMemset(inexact_dev + w.id, 0, sizeof(int)));      // it may be exact again
    }
};

inline void add_slot(lr_engine* e, const std::string& name, std::vector<int64_t> shape, void* dst, int ld_dst, int cols_dst,
              int dst_dtype, int mode, double std_, double offset) {
    Slot s;
    s.name = name;
    s.shape = shape;
    if (shape.size() == 1) { s.rows = 1; s.cols = (int)shape[0]; }
    else { s.rows = (int)shape[0]; int64_t c = 1; for (size_t i = 1; i < shape.size(); ++i) c *= shape[i]; s.cols = (int)c; }
    s.dst = dst; s.ld_dst = ld_dst; s.cols_dst = cols_dst; s.dst_dtype = dst_dtype; s.mode = mode;
    s.std_ = std_; s.offset = offset;
    if (dst_dtype == DT_F16 || dst_dtype == DT_BF16) {
        for (Weight& w : e->weights)
            if ((char*)dst >= w.hi && (char*)dst < w.hi + w.bytes) { s.weight = &w; if (w.lo) s.lo_dst = w.lo + ((char*)dst - w.hi); break; }
    }
    e->index[name] = (int)e->slots.size();
    e->slots.push_back(s);
}

inline float* falloc(lr_engine* e, size_t n) { return (float*)e->dalloc(n * 4, true); }
inline Weight* oalloc(lr_engine* e, size_t n) {
    Weight w;
    w.hi = (char*)e->dalloc(n * 2, true);
    if (e->created.prec) w.lo = (char*)e->dalloc(n * 2, true);
    w.bytes = n * 2; w.id = (int)e->weights.size();
    e->weights.push_back(w);
    return &e->weights.back();
}

inline void vec_slot(lr_engine* e, const std::string& name, std::vector<int64_t> shape, float* dst, double std_, double off) {
    int64_t n = 1; for (auto v : shape) n *= v;
    add_slot(e, name, shape, dst, (int)n, (int)n, DT_F32, PACK_PLAIN, std_, off);
    // 1-D view of multi-dim vectors (glb_GN [1,1,4H]) : force [1, n]
    e->slots.back().rows = 1; e->slots.back().cols = (int)n;
}

inline void register_clip(lr_engine* e, const std::string& cp) {
    const lr_model_desc& d = e->d;
    const int Hc = d.clip_hidden, Mc = d.clip_mlp;
    const int od = e->op_dt;
    e->cls = falloc(e, Hc);
    vec_slot(e, cp + "embeddings.class_embedding", {Hc}, e->cls, 0.02, 0);
    e->patch_w = oalloc(e, (size_t)Hc * e->Kpad);
    add_slot(e, cp + "embeddings.patch_embedding.weight", {Hc, 3, d.clip_patch, d.clip_patch}, e->patch_w->hi, e->Kpad, e->Kpad, od,
             PACK_PLAIN, 0.02, 0);
    e->pos = falloc(e, (size_t)e->T * Hc);
    add_slot(e, cp + "embeddings.position_embedding.weight", {e->T, Hc}, e->pos, Hc, Hc, DT_F32, PACK_PLAIN, 0.02, 0);
    e->pre_w = falloc(e, Hc); e->pre_b = falloc(e, Hc);
    vec_slot(e, cp + "pre_layrnorm.weight", {Hc}, e->pre_w, 0.05, 1.0);
    vec_slot(e, cp + "pre_layrnorm.bias", {Hc}, e->pre_b, 0.02, 0);
    e->cl.resize(d.clip_layers);
    for (int l = 0; l < d.clip_layers; ++l) {
        ClipLayer& c = e->cl[l];
        const std::string p = cp + "encoder.layers." + std::to_string(l) + ".";
        c.qkv_w = oalloc(e, (size_t)3 * Hc * Hc); c.qkv_b = falloc(e, 3 * Hc);
        const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
        for (int i = 0; i < 3; ++i) {
            add_slot(e, p + "self_attn." + nm[i] + ".weight", {Hc, Hc}, c.qkv_w->hi + (size_t)i * Hc * Hc * 2, Hc, Hc, od,
                     PACK_PLAIN, 0.02, 0);
            vec_slot(e, p + "self_attn." + nm[i] + ".bias", {Hc}, c.qkv_b + i * Hc, 0.02, 0);
        }
        c.out_w = oalloc(e, (size_t)Hc * Hc); c.out_b = falloc(e, Hc);
        add_slot(e, p + "self_attn.out_proj.weight", {Hc, Hc}, c.out_w->hi, Hc, Hc, od, PACK_PLAIN, 0.02, 0);
        vec_slot(e, p + "self_attn.out_proj.bias", {Hc}, c.out_b, 0.02, 0);
        c.ln1_w = falloc(e, Hc); c.ln1_b = falloc(e, Hc); c.ln2_w = falloc(e, Hc); c.ln2_b = falloc(e, Hc);
        vec_slot(e, p + "layer_norm1.weight", {Hc}, c.ln1_w, 0.05, 1.0);
        vec_slot(e, p + "layer_norm1.bias", {Hc}, c.ln1_b, 0.02, 0);
        c.fc1_w = oalloc(e, (size_t)Mc * Hc); c.fc1_b = falloc(e, Mc);
        add_slot(e, p + "mlp.fc1.weight", {Mc, Hc}, c.fc1_w->hi, Hc, Hc, od, PACK_PLAIN, 0.02, 0);
        vec_slot(e, p + "mlp.fc1.bias", {Mc}, c.fc1_b, 0.02, 0);
        c.fc2_w = oalloc(e, (size_t)Hc * Mc); c.fc2_b = falloc(e, Hc);
        add_slot(e, p + "mlp.fc2.weight", {Hc, Mc}, c.fc2_w->hi, Mc, Mc, od, PACK_PLAIN, 0.02, 0);
        vec_slot(e, p + "mlp.fc2.bias", {Hc}, c.fc2_b, 0.02, 0);
        vec_slot(e, p + "layer_norm2.weight", {Hc}, c.ln2_w, 0.05, 1.0);
        vec_slot(e, p + "layer_norm2.bias", {Hc}, c.ln2_b, 0.02, 0);
    }
}

inline void upload_rope_tables(lr_engine* e) {
    e->inv_s = falloc(e, LR_MAX_HALF_HEAD); e->inv_l = falloc(e, LR_MAX_HALF_HEAD);
    LR_HIP_CHECK(hipMemcpy(e->inv_s, e->d.inv_freq_short, sizeof(e->d.inv_freq_short), hipMemcpyHostToDevice));
    LR_HIP_CHECK(hipMemcpy(e->inv_l, e->d.inv_freq_long, sizeof(e->d.inv_freq_long), hipMemcpyHostToDevice));
}


// One slot of the per-forward table ring: taking it waits until the pass that used it NSLOT passes ago has read it (bounds host
// run-ahead to NSLOT passes); the caller fills host(), commit() mirrors it to dev() on st.
struct TableSlot {
    lr_engine* h; int i;
    explicit TableSlot(lr_engine* e) : h(e), i(e->slot_i) {
        e->slot_i = (i + 1) % lr_engine::NSLOT;
        if (e->tab_used[i]) LR_HIP_CHECK(hipEventSynchronize(e->tab_ev[i]));
    }
    char* host() const { return h->tab_host + (size_t)i * h->tab_bytes; }
    char* dev() const { return h->tab_dev + (size_t)i * h->tab_bytes; }
    void commit(hipStream_t st) const {
        LR_HIP_CHECK(hipMemcpyAsync(dev(), host(), h->tab_bytes, hipMemcpyHostToDevice, st));
        LR_HIP_CHECK(hipEventRecord(h->tab_ev[i], st));
        h->tab_used[i] = true;
    }
};

// Argument checks the entry points share; who = the entry's name, the prefix of its message.
inline void require(bool ok, const char* who, const char* what) { if (!ok) throw std::invalid_argument(std::string(who) + what); }
inline void check_batch(const lr_engine* h, int B, const char* who) { require(B >= 1 && B <= h->d.max_batch, who, ": batch exceeds max_batch"); }
inline void check_seq(const lr_engine* h, int S, const char* who) { require(S >= 1 && S <= h->d.max_seq, who, ": sequence exceeds max_seq"); }
inline void check_crops(const lr_engine* h, int n, const char* who) { require(n >= 2 && n <= h->d.max_crops, who, ": n_crops exceeds max_crops"); }
inline void check_pix_dtype(int dt, const char* who) { require(dt == LR_DT_F32 || dt == LR_DT_BF16, who, ": pixel dtype must be F32 or BF16"); }
inline int op_dtype(int lr_dt) { return lr_dt == LR_DT_F16 ? DT_F16 : DT_BF16; }      // LR_DT_* of an operand -> DT_*

template <typename F> int guarded(lr_engine* e, F&& f) {
    try {
        if (e) LR_HIP_CHECK(hipSetDevice(e->device));
        f();
        return LR_OK;
    } catch (const std::invalid_argument& ex) {
        (e ? e->err : g_create_error) = ex.what();
        return LR_EINVAL;
    } catch (const std::logic_error& ex) {
        (e ? e->err : g_create_error) = ex.what();
        return LR_ESTATE;
    } catch (const std::exception& ex) {
        (e ? e->err : g_create_error) = ex.what();
        return LR_EHIP;
    }
}

// An activation buffer as the GEMM or attention launch behind it reads it.  Producers (norms, im2col and the gathers, operand-out /
// SwiGLU / RoPE epilogues, the in-place re-encode) return or fill one; consumers take one and refuse a layout their form does not read.
enum : int { LAY_SINGLE = 0, LAY_LO16 = 1, LAY_LO8 = 2 };      // rows of `width` | [hi | 16-bit lo] | [hi | block-scaled e4m3 lo]
struct Operand {
    void* p = nullptr;
    int width = 0, rows = 0;               // LOGICAL columns (the consumer's K) and rows
    int lay = LAY_SINGLE;
    const unsigned char* sc = nullptr;     // LAY_LO8: the block scales of the residual half (one of lr_engine::sc)
    bool hi8 = false;                      // LAY_LO8: ... together with the e4m3 copy of the hi half (third e4m3 segment, lr_engine::aexp2)
    int ld() const { return lay == LAY_SINGLE ? width : 2 * width; }
};
// what every producer without a one-byte residual path writes at form f
inline Operand operand16(void* p, int width, int rows, Form f) { return Operand{p, width, rows, f.prec ? LAY_LO16 : LAY_SINGLE}; }
// A consumer at form f reads single rows or [hi | lo] rows, nothing else: a site override (lr_set_precision_sites) on a single-pass
// layer range would otherwise have a single-pass reader walk [hi | lo] rows at half their stride, silently.
inline void check_layout(const Operand& x, Form f, const char* reader) {
    if ((x.lay != LAY_SINGLE) != (f.prec != 0))
        throw std::logic_error(std::string(reader) + (f.prec ? ": a split-operand site reads single rows" : ": a single-pass site reads [hi | lo] rows") +
                               " (lr_set_precision_map / lr_set_precision_sites: neighbouring sites must agree on split operands)");
}

// Split-operand mode: callers pass LOGICAL shapes; here A becomes [A_hi | A_lo] (K doubled, W re-read from column 0) and an
// operand-typed output becomes [C_hi | C_lo].
// With desc.precise == 2 the residual pass of a GEMM that runs on the deep-pipelined kernel is made in e4m3: the residual half of
// A arrives as block-scaled e4m3 from its producer (norms, SwiGLU / operand-out epilogues: LAY_LO8) or is re-encoded in place
// (stream-ordered, right here: every operand buffer feeds exactly one GEMM after it is produced), and W's e4m3 twin is prepared on
// first use in the rows of its residual buffer (exact weights only; one synchronisation per weight).
// apply_prec_base only rewrites the parameters (no side effects); commit_lo8 commits the e4m3 form right before the launch.
inline void apply_prec_base(const Weight& W, Form f, GemmParams& p) {      // p.W == W.hi
    if (!f.prec) return;
    p.kw = p.K; p.K *= 2; p.lda *= 2;
    if (W.inexact) {     // weights not exact in the operand type
        p.Wlo = W.lo;
        p.K = 3 * p.kw;
    }
    if (p.epi == EPI_OUT_OP || p.epi == EPI_SWIGLU_OP || p.epi == EPI_ROPE_OP) { p.split = p.ldc; p.ldc *= 2; }
}
// The choice must not depend on M: a row's reward has to be bit-identical whatever else is in the batch (sharding across GPUs
// must not change a preference), so every eligible GEMM takes this form -- on the deep-pipelined kernel -- at any row count.
inline bool lo8_eligible(const lr_engine* e, Form f, const GemmParams& p) {      // p after apply_prec_base
    if (!f.lo8 || p.kw <= 0) return false;
    const bool aligned = p.N % 8 == 0 && p.ldc % 8 == 0 && (((uintptr_t)p.C) & 15) == 0 && (!p.bias || (((uintptr_t)p.bias) & 15) == 0);
    return aligned && p.kw % 128 == 0 && p.ldw == p.kw && (e->gemm_tile < 0 || e->gemm_tile == 6);
}
// e4m3 twin(s) of weight W [N, K], placed as Weight::Lo8 says; synchronous.  lr_finalize calls it for every GEMM weight it knows
// (prepare_twins below), the launch path only as a fallback (weights re-uploaded after lr_finalize).
inline void ensure_lo8_twin(lr_engine* e, Weight& W, int N, int K, int ldw, hipStream_t st) {
    Weight::Lo8& t = W.lo8;
    if (t.ready) return;
    if (!e->amax_word) e->amax_word = (unsigned*)e->dalloc(256, false);
    t.E = t.E2 = 127;
    if (t.where == Weight::OWN) {
        t.E = prepare_weight_e4m3(W.hi, ldw, K, N, t.buf, e->op_dt, e->amax_word, st);
    } else if (W.inexact) {
        const size_t need = (size_t)N * ldw * 2;
        if (need > e->w8tmp_cap) {
            if (e->w8tmp) e->dfree(e->w8tmp, e->w8tmp_cap);
            e->w8tmp_cap = need; e->w8tmp = e->dalloc(need, false);
        }
        if (!t.buf) { t.buf = e->dalloc(need, true); t.where = Weight::PAIR; }
        LR_HIP_CHECK(hipMemcpyAsync(t.buf, W.lo, need, hipMemcpyDeviceToDevice, st));      // the 16-bit residuals: converted in the copy
        prepare_weight_e4m3_pair(W.hi, t.buf, ldw, K, N, e->w8tmp, e->op_dt, e->amax_word, st, &t.E, &t.E2);
    } else {
        t.E = prepare_weight_e4m3(W.hi, ldw, K, N, W.lo, e->op_dt, e->amax_word, st);
    }
    t.ready = true;
}
// scale arrays (and the hi-half row exponents) large enough for an operand of `rows` x K; presized at lr_finalize (prepare_twins)
inline void ensure_aexp(lr_engine* e, size_t rows, size_t K) {
    const size_t need = lo8_scale_bytes((int)rows, (int)K);
    if (need > e->sc_cap) {
        // (presized at lr_finalize; a growth during a forward is a fallback: hipMalloc synchronises the device, and the fill is
        //  ordered for every stream by the device-wide synchronisation behind it)
        e->sc_cap = (need + 65535) & ~(size_t)65535;
        for (int i = 0; i < 2; ++i) {
            e->sc[i] = (unsigned char*)e->dalloc(e->sc_cap, false);
            LR_HIP_CHECK(hipMemset(e->sc[i], 127, e->sc_cap));           // rows beyond M of a last tile read these: any finite scale
        }
        LR_HIP_CHECK(hipDeviceSynchronize());
    }
    if (rows > e->aexp2_cap) {
        e->aexp2_cap = (rows + 4095) & ~(size_t)4095;
        e->aexp2 = (int*)e->dalloc(e->aexp2_cap * 4, false);
    }
}
// the array the next producer of one-byte residuals writes its scales to
inline unsigned char* next_scales(lr_engine* e) { e->sc_i ^= 1; return e->sc[e->sc_i]; }

// x's residual half as block-scaled e4m3 (hi8: with the e4m3 copy of its hi half): nothing to do on rows that carry them already, else
// one in-place pass.  Idempotent, so the adapter's t GEMM and the main GEMM, which read the same rows, both call it.
inline void encode_lo8(lr_engine* e, Operand& x, bool hi8, hipStream_t st) {
    if (x.lay == LAY_LO8 && (!hi8 || x.hi8)) return;
    if (x.lay == LAY_LO8) throw std::logic_error("operand buffer already carries e4m3 residuals without the e4m3 copy of its hi half");
    unsigned char* sc = next_scales(e);
    launch_quantize_lo_inplace(x.p, x.ld(), x.width, x.rows, sc, e->op_dt, st, hi8 ? e->aexp2 : nullptr);
    x.lay = LAY_LO8; x.sc = sc; x.hi8 = hi8;
}
// p: after apply_prec_base, lo8_eligible, reading x.  next_hi8: the GEMM that reads the same rows next (the main GEMM behind an
// adapter's t GEMM) needs the e4m3 copy of the hi half, so the one in-place encoding pass writes it now.
inline void commit_lo8(lr_engine* e, Weight& W, GemmParams& p, Operand& x, hipStream_t st, bool next_hi8 = false) {
    // Weights inexact in the operand type (Wlo set by apply_prec_base: a merged LoRA adapter, fp32-trained weights): a third
    // e4m3 segment, A_hi8 x e4m3(W_lo)^T, replaces the 16-bit [x_hi] x [W_lo] segment (2x instead of 3x the single pass).
    // Adapter matrices (Weight::OWN) keep the 16-bit third segment: their twin holds e4m3(W) only.
    const bool inexact = p.Wlo != nullptr, own = W.lo8.where == Weight::OWN;
    const bool third8 = inexact && !own;
    ensure_lo8_twin(e, W, p.N, p.kw, p.ldw, st);
    ensure_aexp(e, (size_t)p.M, (size_t)p.kw);
    encode_lo8(e, x, third8 || next_hi8, st);
    p.aexp = x.sc;
    if (own) p.Wlo16 = inexact ? W.lo : nullptr;
    p.Wlo = W.lo8_rows();
    p.wexp = W.lo8.E;
    p.aexp2 = third8 ? e->aexp2 : nullptr;
    p.wexp2 = W.lo8.E2;
}
// An attention launch at form f reading q, k, v from the rows of `qkv` (p in LOGICAL strides); returns O as the GEMM behind it reads it.
inline Operand apply_prec(const lr_engine* e, Form f, AttnParams& p, const Operand& qkv, int o_rows) {
    check_layout(qkv, f, "attention");
    if (qkv.lay == LAY_LO8) throw std::logic_error("attention reads 16-bit residuals: its operand carries e4m3 residuals");
    const Operand o = operand16(p.O, p.ldo, o_rows, f);
    if (!f.prec) return o;
    p.lo_off = p.ldq; p.ldq *= 2;
    p.o_split = p.ldo; p.ldo *= 2;
    // strict stages (16-bit residual passes: the probe's yardstick, and what an amplifying weight set is locked to) keep the exact
    // softmax maximum; stages in the default form take the lazy one (attention.hip; -14 % per launch)
    // (A/B switches for tools/outlier_fp64_probe.py, read once: LR_ATT_LAZY_T overrides the default-form stages' threshold, LR_ATT_LAZY_T_STRICT the strict stages')
    static const float t_def = [] { const char* v = getenv("LR_ATT_LAZY_T"); return v ? (float)atof(v) : -1.f; }();
    static const float t_strict = [] { const char* v = getenv("LR_ATT_LAZY_T_STRICT"); return v ? (float)atof(v) : 0.f; }();
    p.lazy_t = f.lo8 ? (t_def >= 0.f ? t_def : e->att_lazy_t) : (t_strict > 0.f ? t_strict : e->att_lazy_t_strict);
    return o;
}

// W8A8 mode: quantise the rows of A, make sure W has its e4m3 twin, launch the e4m3 form.  Like lo8_eligible, the choice never
// depends on M.  Returns false when this GEMM has to stay in 16 bits (K % 128 != 0, unaligned output).
inline bool w8a8_eligible(const lr_engine* e, const GemmParams& p) {
    const bool aligned = p.N % 8 == 0 && p.ldc % 8 == 0 && (((uintptr_t)p.C) & 15) == 0 && (!p.bias || (((uintptr_t)p.bias) & 15) == 0);
    return e->w8a8 && aligned && p.K % 128 == 0 && p.lda % 8 == 0 && p.ldw % 8 == 0 && (e->gemm_tile < 0 || e->gemm_tile == 6);
}
inline void ensure_w8a8_twin(lr_engine* e, Weight& W, int N, int K, int ldw, hipStream_t st) {
    Weight::W8& t = W.w8;
    if (t.ready) return;
    if (!t.q) { t.q = e->dalloc((size_t)N * K, true); t.scale = (float*)e->dalloc((size_t)N * 4, true); }      // (N, K: fixed per weight)
    launch_quantize_rows_fp8(W.hi, ldw, K, N, t.q, K, t.scale, e->op_dt, st);
    t.ready = true;
}
inline void ensure_q8(lr_engine* e, size_t rows, size_t K) {
    const size_t need = rows * K;
    if (need > e->q8_cap) { e->q8_cap = (need + (1u << 20)) & ~(size_t)((1u << 20) - 1); e->q8 = e->dalloc(e->q8_cap, false); }
    if (rows > e->q8s_cap) { e->q8s_cap = (rows + 4095) & ~(size_t)4095; e->q8s = (float*)e->dalloc(e->q8s_cap * 4, false); }
}
// lr_finalize: twins of every GEMM weight {W, N, K} with K % 128 == 0 and scratch for `rows` operand rows, so that no forward has to
// synchronise or allocate (weights re-uploaded afterwards fall back to preparation at their first launch).
struct GemmWeight { Weight* W; int N, K; size_t rows; };
inline void prepare_twins(lr_engine* e, const std::vector<GemmWeight>& ws) {
    if (!e->created.lo8 && !e->w8a8) return;
    for (const GemmWeight& g : ws) {
        if (!g.W || g.K % 128) continue;
        if (e->created.lo8) { ensure_lo8_twin(e, *g.W, g.N, g.K, g.K, 0); ensure_aexp(e, g.rows, (size_t)g.K); }
        else { ensure_w8a8_twin(e, *g.W, g.N, g.K, g.K, 0); ensure_q8(e, g.rows, (size_t)g.K); }
    }
    LR_HIP_CHECK(hipStreamSynchronize(0));
}

inline bool launch_w8a8(lr_engine* e, Weight& W, GemmParams p, hipStream_t st) {
    if (!w8a8_eligible(e, p)) return false;
    ensure_w8a8_twin(e, W, p.N, p.K, p.ldw, st);
    ensure_q8(e, (size_t)p.M, (size_t)p.K);
    launch_quantize_rows_fp8(p.A, p.lda, p.K, p.M, e->q8, p.K, e->q8s, e->op_dt, st);
    p.A = e->q8; p.W = W.w8.q; p.lda = p.K; p.ldw = p.K;
    p.ascale = e->q8s; p.wscale = W.w8.scale;
    launch_gemm_bt8_fp8(p, e->op_dt, st);
    return true;
}

// One linear layer y = act(x W^T + bias), described ONCE, in LOGICAL shapes: the same object tells the producer of x whether to write
// one-byte residuals (lo8_scales) and launches the GEMM (linear() below), so the two cannot disagree about the rows between them.
struct Linear {
    Weight* W; const float* bias; int N, K;           // W [N, K]
    int epi, act;
    const Lora* L = nullptr;               // un-merged adapter, or null / k2 == 0
    const float* rope_cs = nullptr; int rope_cols = 0, rope_hd = 0;     // EPI_ROPE_OP (GemmParams)
    bool adapter() const { return L && L->k2 > 0; }
    bool rope_tiles_ok() const { return rope_cols % 256 == 0; }        // the fused RoPE epilogue rotates whole 256-column tiles
    int out_cols() const { return epi == EPI_SWIGLU_OP ? N / 2 : N; }
    GemmParams params(const lr_engine* e, const void* A, void* C, int M) const {
        GemmParams p{A, W->hi, C, bias, M, N, K, K, K, out_cols(), epi, act, rope_cs, rope_cols, rope_hd};      // the kernels' view: raw pointers
        p.sched_mem = e->sched_mem;
        return p;
    }
    // For the producer of this GEMM's operand x [M, K] (a norm kernel, the epilogue of the GEMM in front): where to put x's block
    // scales if this GEMM, at form f, will take the e4m3 residual form with exact weights (it then finds its operand encoded: no
    // in-place pass), else null (the producer writes 16-bit residuals as usual).
    unsigned char* lo8_scales(lr_engine* e, Form f, int M) const {
        if (!f.lo8 || (epi == EPI_ROPE_OP && !rope_tiles_ok())) return nullptr;       // (no fused RoPE: qkv_rope runs another GEMM)
        GemmParams probe = params(e, nullptr, nullptr, M);
        apply_prec_base(*W, f, probe);
        if (!lo8_eligible(e, f, probe) || probe.Wlo) return nullptr;
        ensure_aexp(e, (size_t)M, (size_t)K);
        return next_scales(e);
    }
};

// y = norm(x) as the operand of `reader` at form f (reader == null: 16-bit residuals whatever reads them).
inline Operand norm_rows(lr_engine* e, hipStream_t st, Form f, const Linear* reader, const float* x, const float* w, const float* b, void* y,
                         int rows, int H, float eps, int group = 1) {
    Operand o = operand16(y, H * group, rows / group, f);
    unsigned char* sc = reader ? reader->lo8_scales(e, f, o.rows) : nullptr;
    launch_norm_rows(x, w, b, y, rows, H, eps, e->op_dt, st, f.prec, group, sc);
    if (sc) { o.lay = LAY_LO8; o.sc = sc; }
    return o;
}

// Runs l on the rows of x at form f, C = the output buffer; returns the output as its reader finds it (operand-typed epilogues).
// With an adapter: t = x A^T first (always on the deep-pipelined kernel, in the same operand form as the main GEMM -- they read the
// same rows of x), then the main GEMM with the K-extension.
// next / next_f: the linear that reads this one's output as its operand and the form of ITS site (default: f): they decide whether the
// epilogue writes one-byte residuals -- the CONSUMER's form and weights, not this GEMM's.  The kernel must be the deep-pipelined one.
inline Operand linear(lr_engine* e, hipStream_t st, Form f, const Linear& l, Operand& x, void* C, const Linear* next = nullptr, Form next_f = Form{-1, -1}) {
    check_layout(x, f, "GEMM");
    if (next_f.prec < 0) next_f = f;
    const bool op_out = l.epi == EPI_OUT_OP || l.epi == EPI_SWIGLU_OP || l.epi == EPI_ROPE_OP;
    Operand y = op_out ? operand16(C, l.out_cols(), x.rows, f) : Operand{};
    GemmParams p = l.params(e, x.p, C, x.rows), t{};
    if (l.adapter()) {
        if (e->w8a8) throw std::logic_error("W8A8 mode runs merged weights only (no un-merged adapters)");
        const int k2 = l.L->k2;
        t = Linear{l.L->A, nullptr, k2, l.K, EPI_OUT_OP, ACT_NONE}.params(e, x.p, e->lt, x.rows);
        apply_prec_base(*l.L->A, f, t);
        p.A2 = e->lt; p.lda2 = k2 * (1 + f.prec); p.W2 = l.L->B->hi; p.ldw2 = k2; p.k2 = k2;
        if (l.L->B->inexact) p.W2lo = l.L->B->lo;
    } else if (launch_w8a8(e, *l.W, p, st)) return y;
    apply_prec_base(*l.W, f, p);
    const bool lo8 = lo8_eligible(e, f, p) && (!l.adapter() || lo8_eligible(e, f, t));
    if (x.lay == LAY_LO8 && !lo8) throw std::logic_error("operand pre-encoded in e4m3 for a GEMM that takes the 16-bit form");
    if (l.adapter()) {
        if (lo8) commit_lo8(e, *l.L->A, t, x, st, p.Wlo != nullptr);
        launch_gemm_bt(t, e->op_dt, 6, st);
    }
    if (lo8) commit_lo8(e, *l.W, p, x, st);
    if (next && next_f.prec == f.prec && (l.epi == EPI_OUT_OP || l.epi == EPI_SWIGLU_OP) && p.split > 0 &&        // (a single-pass neighbour: no residual half at all)
        (p.A2 || gemm_bt_is_deep(p, e->gemm_tile)) && (e->gemm_tile < 0 || e->gemm_tile == 6))
        p.oexp = next->lo8_scales(e, next_f, p.M);
    launch_gemm_bt(p, e->op_dt, e->gemm_tile, st);
    if (p.oexp) { y.lay = LAY_LO8; y.sc = p.oexp; }
    return y;
}

// qkv projection with RoPE on q, k (l: EPI_ROPE_OP; v = the columns behind rope_cols): fused in the GEMM epilogue when the
// deep-pipelined kernel runs, else an fp32 projection + launch_rope_split.
// qkv32: the pre-RoPE fp32 projections of up to cap_rows rows: only the fallback needs them, so they are allocated on its first use
// (decoder: 3.1 GB at B = 32).
inline Operand qkv_rope(lr_engine* e, hipStream_t st, Form f, const Linear& l, Operand& x, void* qkv, float*& qkv32, size_t cap_rows) {
    GemmParams probe = l.params(e, x.p, qkv, x.rows);
    apply_prec_base(*l.W, f, probe);
    if (l.rope_tiles_ok() && (l.adapter() || w8a8_eligible(e, probe) || lo8_eligible(e, f, probe) || gemm_bt_is_deep(probe, e->gemm_tile)))
        return linear(e, st, f, l, x, qkv);
    if (!qkv32) qkv32 = (float*)e->dalloc((cap_rows + 256) * l.N * 4, false);
    linear(e, st, f, Linear{l.W, l.bias, l.N, l.K, EPI_OUT_F32, ACT_NONE, l.L}, x, qkv32);
    launch_rope_split(qkv32, l.rope_cs, qkv, x.rows, l.rope_cols, l.N - l.rope_cols, l.rope_hd, e->op_dt, st, f.prec);
    return operand16(qkv, l.N, x.rows, f);
}

// Adapter slots of one linear `mod` (checkpoint names mod.lora_A.weight [r, K], mod.lora_B.weight [n_rows, r]); part / parts: this
// adapter's place among the stacked adapters of a fused linear; b_row0: first row of the fused weight this part owns (B is block
// diagonal); pack_mode / aux_*: the row packing of the base weight's slot.  B must arrive pre-scaled by lora_alpha / r.
inline void register_lora(lr_engine* e, Lora& L, const std::string& mod, int N_fused, int K, int part, int parts, int n_rows, int b_row0,
                          int pack_mode, int aux_d = 0, int aux_hd = 0) {
    const int r = e->d.lora_rank, rp = e->lora_rp, od = e->op_dt;
    if (part == 0) {
        L.k2 = parts * rp;
        L.A = oalloc(e, (size_t)L.k2 * K);
        L.B = oalloc(e, (size_t)N_fused * L.k2);
        if (e->created.lo8) L.A->lo8 = Weight::Lo8{Weight::OWN, e->dalloc((size_t)L.k2 * K * 2, true)};
        e->lora_k2max = std::max(e->lora_k2max, L.k2);
    }
    add_slot(e, mod + ".lora_A.weight", {r, K}, L.A->hi + (size_t)part * rp * K * 2, K, K, od, PACK_PLAIN, 0.02, 0);
    add_slot(e, mod + ".lora_B.weight", {n_rows, r}, L.B->hi + ((size_t)b_row0 * L.k2 + (size_t)part * rp) * 2, L.k2, r, od, pack_mode, 0.02, 0);
    e->slots.back().aux_d = aux_d; e->slots.back().aux_hd = aux_hd;
}


// ---- shared image prefix: layout of a cache ----
// [256-byte head: int {0, V, image slots among the shared tokens} | per decoder layer l < nl: the qkv rows of the n_shared shared
//  positions exactly as that layer's attention site reads them (post-RoPE, [hi | lo] where the site's form is split; the row stride of
//  the qkv buffer, so the attention kernel's per-thread offsets serve both sources) | ev: V projected image rows, fp32]
struct PrefixLayout { std::vector<size_t> layer; size_t ev = 0, total = 0; int nl = 0; };

// engine.hip: THE pre-norm decoder pass of the three backbones and the two prefix entries (x, cs, tstat prepared by the caller) over B
// sequences of S rows; mask [B, S] or null (every row valid).
// gather: 0 = every row through every layer; 1 / 2 = only the row of each sequence the reward is read from is wanted afterwards
// (1: its last valid position, tstat[4 b]; 2: position S - 1): the LAST layer then runs its attention, o_proj and MLP for those B
// rows only (rw_model:408-421 reads one row per sample) and leaves them in h->xg [B, hidden]; returns true when it did.
// KV sink (kv_out): layer l's projection writes its rows to kv_out + layout->layer[l] instead of h->qkv, its attention reads them there,
// and the last layer stops behind its projection.  KV prefix (kv_shared): the n_shared rows at kv_shared + layout->layer[l] sit in
// front of every sequence's own keys.  A pass with neither alone passes the first valid key (tstat + 1) and runs LR_ATT_EMU_LO8.
struct DecoderPass {
    const int64_t* mask; int B, S;
    int gather = 0;
    const PrefixLayout* layout = nullptr;
    char* kv_out = nullptr;
    const char* kv_shared = nullptr; int n_shared = 0;
};
bool run_decoder_stack(lr_engine* h, hipStream_t st, const DecoderPass& p);
void alloc_gather_ws(lr_engine* h);
// engine.hip, for both finalizers: the decoder's workspace of Rl rows (x .. cs, lt, pos_ids, img_row, in this order) and its e4m3-twin entries
void alloc_decoder_ws(lr_engine* h, size_t Rl);
void push_decoder_weights(const lr_engine* h, std::vector<GemmWeight>& ws, size_t Rl);
// engine.hip: rw_model:398-406 -- SkipCA for every token (o: per-token term, u: per-sample term, either may be null), masked mean
// pooling into h->hL, value head.  Vb / voff: image rows of every sample in h->ev (host), Vmax = their maximum.
void run_mean_pool_head(lr_engine* h, hipStream_t st, const int64_t* attention_mask, int B, int S, const int* voff_host, int Vmax,
                        const float* u, bool final_norm, float* rewards_out);
void alloc_mean_pool(lr_engine* h, size_t rows, size_t vcap);
// qwen.hip
void build_weight_table_qwen(lr_engine* e);
void validate_desc_qwen(const lr_model_desc& d);
void finalize_qwen(lr_engine* h);
