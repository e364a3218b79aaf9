// trainer.hip -- the training step of the RPN, host code only: the counterpart of the reference's trainer.py:54-69 (compile with
// Adam(1e-5) and loss=[reg_loss, cls_loss], then fit).  The kernels, their launchers and the loss / Adam / BatchNorm forms are in
// train_kernels.hip (train_head.h), train_backbone_kernels.hip / train_backbone_x3_kernels.hip (train_backbone.h) and
// train_mnv2_kernels.hip (train_mnv2.h).
//
// rpn_head_trainer_create trains the head (rpn_conv, rpn_reg, rpn_cls) on a frozen backbone:
//   backbone (the handle's own ops and precision) -> X (B,F,F,Cin) float32
//   rpn_conv (exact float32, ReLU) -> S (P,512), P = B F F;  fused 1x1 head -> reg (P,4K) linear | cls (P,K) sigmoid
//   losses + their gradients;  the head's backward;  rpn_conv's weight and bias gradient;  Adam over every trained tensor in one launch
// rpn_model_trainer_create also trains the VGG16 convs from a given one up (the reference's Keras base model is trainable): the whole
// VGG16 forward in exact float32 from the trainer's weights (backbone_forward) and, after the head's backward, the backbone's
// (backbone_backward).  On a MobileNetV2 handle it trains the stride-16 blocks from a given expand conv up, rpn_model_trainer_create_full
// the whole model, with BatchNorm in training mode: the layers below run frozen on the handle's ops (BatchNorm folded), the trained
// ones in exact float32 from the trainer's unfolded parameters (mn_forward / mn_backward).
//
// Every device pointer lives in TrainerDevice and every allocation in one list (dev_alloc / trainer_free).  Every parameter the C ABI
// names is an entry of one table (Param): set / get / gradient / "was it set" are a lookup (param_access) and one copy (param_copy).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "conv_kernels.h"
#include "rpn_common.h"
#include "train_backbone.h"
#include "train_head.h"
#include "train_mnv2.h"

using namespace rpn;

namespace {

constexpr int kMnMax = 40;                      // MobileNetV2's convs up to block_13_expand (mn_table())

// ---- the parameter table --------------------------------------------------------------------------------------------------------
// The flat float32 buffers a parameter can live in.  kMaster: the trained tensors (d.w / host[kMaster]; d.g, d.m, d.v in the same
// layout: the gradients, Adam's m and v); kFrozen: the VGG16 convs below the trained span; kBnState: the moving mean | variance of the
// trained BatchNorms (state outside Adam's buffer); kBnStep: the statistics a step normalised with (device only, never set or read).
enum Store { kMaster, kFrozen, kBnState, kBnStep, kStores };

// One named slice: rows x len floats at `off` of its store, `stride` floats from row to row (the rpn_reg | rpn_cls columns of the fused
// head matrix are strided; everything else is one row).  The caller's array is always dense (rows, len).
struct Param {
    std::string layer;                          // the layer's name in messages
    int store;
    size_t off;
    int rows, len, stride;
    bool loaded;                                // set through the C ABI at least once
};

// Table order = the flat layout of kMaster (gradients, Adam's m and v and saved states depend on it):
//   rpn_conv kernel (3,3,cin,512) | rpn_conv bias | head kernel (512, 5K): rpn_reg columns, then rpn_cls | head bias (5K)
//   a trained VGG16 conv: kernel HWIO | bias (the frozen ones the same in kFrozen)
//   a trained MobileNetV2 conv: kernel (at a multiple of 4 floats: the kernels read these slices as float4; every slice's length is a
//   multiple of 4) | gamma | beta; its moving mean | variance adjacent in kBnState, its step's mean | var | rstd in kBnStep
// A layer's entries are adjacent, so entry = the layer's first + a role.
enum HeadParam { kConvK, kConvB, kHeadK, kHeadB, kClsK, kClsB, kHeadParams };   // kHeadK / kHeadB: rpn_reg's slices start the fused head's
enum Role { kKernel = 0, kBias = 1, kGamma = 1, kBeta = 2, kMean = 3, kVar = 4, kStats = 5, kMnRoles = 6 };

// every device pointer of the trainer: all null, or all that the trainer's kind needs allocated (trainer_device)
struct TrainerDevice {
    float *w, *g, *m, *v;
    float *pconv, *phead;
    float *feat, *S, *reg, *cls, *graw, *dz, *dS;
    float *part;
    char *lws;                                   // the losses' workspace (bytes)
    float *wt;                                   // a dgrad's flipped, transposed weights (any trained backbone)
    // the VGG16 backbone
    float *frozen, *pack, *wpart, *img4;
    char *x3img;                                 // the split-float16 dgrad's weight image (the largest trained layer's)
    unsigned *x3meta;                            // 64 words: max bits of a gradient (0) and a kernel (1), the sticky status (2), the pairs {2^t, 2^-t}, {2^s, 2^-s} from word 8
    float *act[13], *pool[13], *ping[2], *grad[2];
    // MobileNetV2
    float *bn, *bstat, *x0, *mpack, *mwpart;
    double *mpart;
    float *mz[kMnMax], *my[kMnMax], *mgr[2], *mt[3];   // my[last] is feat (mn_forward)
};

}  // namespace

struct rpn_head_trainer {
    rpn_model *m = nullptr;
    int cin = 0, F = 0, K = 0, max_batch = 0, nc = 0;
    std::vector<Param> params;
    size_t size[kStores] = {};                  // floats of each store
    std::vector<float> host[kBnStep];           // the stores until the first step moves them to the device
    long long t = 0;                            // applied Adam steps
    int last_B = 0;
    int pending_B = 0;                          // the batch of a forward(train = 1) whose backward has not run yet; 0: none
    const float *pending_imgs = nullptr;        // ... and its d_imgs
    const float *d_tap = nullptr;               // the feature tap of the last forward (d.feat, or the VGG16 span's block5_conv3 output)
    TrainerDevice d{};
    std::vector<void *> allocs;                 // what d points into: every hipMalloc of this trainer
    PackedShape ps_conv{}, ps_head{};
    // ---- the update rule (rpn_head_trainer_set_optimizer; default: Adam alone = launch_adam) ----
    OptimConfig opt;
    OptimDevice optdev;
    // ---- the VGG16 backbone (rpn_model_trainer_create; backbone_*) ----
    // bb_from: the first trained conv (index into kVgg), -1 on a head-only trainer
    int bb_from = -1, img = 0;
    int bw_precision = RPN_PRECISION_F32;        // the backbone backward's products (rpn_head_trainer_set_backward_precision)
    int hs[13] = {};                             // spatial side of each conv's input and output
    PackedShape ps_bb[13]{};
    // ---- MobileNetV2 (rpn_model_trainer_create / _create_full on a MobileNetV2 handle; mn_*) ----
    // mn_from: the first trained layer (index into mn_table(): an expand conv of the stride-16 span, or 0 = Conv1: the whole model),
    // -1: none.  mn_hin / mn_hout: the spatial side of each layer's input and output.
    int mn_from = -1;
    std::string mn_x0;                           // the handle's tensor below the span: the frozen prefix ends there (none from Conv1)
    int mn_hin[kMnMax] = {}, mn_hout[kMnMax] = {};
    PackedShape ps_mn[kMnMax]{};
};

namespace {

const char *kHeadLayers[3] = {"rpn_conv", "rpn_reg", "rpn_cls"};

int layer_index(const char *name)
{
    for (int i = 0; i < 3; ++i)
        if (!strcmp(name, kHeadLayers[i])) return i;
    return -1;
}

// the 13 convs of VGG16 (models/rpn_vgg16.py: keras.applications.VGG16 up to block5_conv3), each 3x3 'same' + ReLU;
// pool: MaxPooling2D(2, 2) 'valid' after the conv
struct VggConv {
    const char *name;
    int cin, cout;
    bool pool;
};
const VggConv kVgg[13] = {{"block1_conv1", 3, 64, false},    {"block1_conv2", 64, 64, true},    {"block2_conv1", 64, 128, false},
                          {"block2_conv2", 128, 128, true},  {"block3_conv1", 128, 256, false}, {"block3_conv2", 256, 256, false},
                          {"block3_conv3", 256, 256, true},  {"block4_conv1", 256, 512, false}, {"block4_conv2", 512, 512, false},
                          {"block4_conv3", 512, 512, true},  {"block5_conv1", 512, 512, false}, {"block5_conv2", 512, 512, false},
                          {"block5_conv3", 512, 512, false}};

int vgg_index(const char *name)
{
    for (int i = 0; i < 13; ++i)
        if (!strcmp(name, kVgg[i].name)) return i;
    return -1;
}

// ---- MobileNetV2: the stem and the inverted-residual blocks, each layer at its own resolution ---------------------------------------
// kind 0: 1x1 expand + BatchNorm + ReLU6, 1: depthwise 3x3 + BatchNorm + ReLU6 (stride 1 'same', or stride 2 behind Keras'
// correct_pad: mn_s2_geom), 2: 1x1 project + BatchNorm (linear) (+ the block's input when res), 3: the stem Conv1, a 3x3 stride-2
// conv from the 3-channel image + BatchNorm + ReLU6 (same padding rule).  No conv has a bias.  Keras names; the BatchNorm layer of
// conv X is "X_BN", Conv1's is "bn_Conv1".  expanded_conv has no expand conv.
constexpr int kMnLayers = kMnMax;
constexpr int kMnSpan = 21;                     // block_7_expand: the first layer at the feature map's own resolution (stride 16)
constexpr float kMnBnEps = 1e-3f, kMnBnMomentum = 0.999f;      // keras.applications.MobileNetV2
struct MnConv {
    std::string name, bn;
    int kind, cin, cout, stride;
    bool res;
};
const std::vector<MnConv> &mn_table()
{
    static const std::vector<MnConv> tab = [] {
        std::vector<MnConv> v;
        // (cin, cout, stride) of block_1 .. block_12 (keras.applications.MobileNetV2, alpha 1; expansion 6)
        const int blk[12][3] = {{16, 24, 2}, {24, 24, 1}, {24, 32, 2}, {32, 32, 1}, {32, 32, 1}, {32, 64, 2},
                                {64, 64, 1}, {64, 64, 1}, {64, 64, 1}, {64, 96, 1}, {96, 96, 1}, {96, 96, 1}};
        v.push_back({"Conv1", "bn_Conv1", 3, 3, 32, 2, false});
        v.push_back({"expanded_conv_depthwise", "expanded_conv_depthwise_BN", 1, 32, 32, 1, false});
        v.push_back({"expanded_conv_project", "expanded_conv_project_BN", 2, 32, 16, 1, false});
        for (int b = 0; b < 12; ++b) {
            const std::string pre = "block_" + std::to_string(b + 1) + "_";
            const int cin = blk[b][0], cout = blk[b][1], stride = blk[b][2];
            v.push_back({pre + "expand", pre + "expand_BN", 0, cin, 6 * cin, 1, false});
            v.push_back({pre + "depthwise", pre + "depthwise_BN", 1, 6 * cin, 6 * cin, stride, false});
            v.push_back({pre + "project", pre + "project_BN", 2, 6 * cin, cout, 1, cin == cout && stride == 1});
        }
        v.push_back({"block_13_expand", "block_13_expand_BN", 0, 96, 576, 1, false});
        return v;
    }();
    return tab;
}

// index of conv `name`, or of the conv whose BatchNorm layer is `name` (with_bn: "<conv>_BN" or the layer's Keras name)
int mn_index(const char *name, bool with_bn = false)
{
    const std::vector<MnConv> &tab = mn_table();
    for (int i = 0; i < kMnLayers; ++i)
        if (tab[i].name == name || (with_bn && (tab[i].name + "_BN" == name || tab[i].bn == name))) return i;
    return -1;
}

size_t mn_kernel_floats(int i)
{
    const MnConv &l = mn_table()[i];
    return l.kind == 1 ? (size_t)9 * l.cout : (l.kind == 3 ? (size_t)27 * l.cout : (size_t)l.cin * l.cout);
}

// ---- table entries and where they live --------------------------------------------------------------------------------------------
// the first entry (the kernel's) of VGG16 conv i (all 13 are in the table) / of MobileNetV2 layer i >= mn_from
int vgg_param(int i) { return kHeadParams + 2 * i; }
int mn_param(const rpn_head_trainer *t, int i) { return kHeadParams + kMnRoles * (i - t->mn_from); }

// one more row-contiguous slice of `len` floats at the end of `store`
void param_append(rpn_head_trainer *t, const std::string &layer, int store, size_t len)
{
    t->params.push_back({layer, store, t->size[store], 1, (int)len, (int)len, store == kBnStep});
    t->size[store] += len;
}

float *store_dev(const rpn_head_trainer *t, int store)
{
    return store == kMaster ? t->d.w : (store == kFrozen ? t->d.frozen : (store == kBnState ? t->d.bn : t->d.bstat));
}
// entry i on the device: the parameter itself (a backbone conv's kernel: the master weights when trained, the frozen constants
// otherwise) and its gradient (kMaster entries only)
float *param_dev(const rpn_head_trainer *t, int i) { return store_dev(t, t->params[i].store) + t->params[i].off; }
float *param_grad(const rpn_head_trainer *t, int i) { return t->d.g + t->params[i].off; }

// One slice between the caller's dense HOST array and its store: the device buffer once the trainer has one (other: a device buffer
// of kMaster's layout instead -- the gradients, Adam's m or v), the host copy before.  On the device a slice moves as the span it
// lies in, staged on the host.
int param_copy(rpn_head_trainer *t, const Param &p, float *user, bool write, float *other, hipStream_t s)
{
    const size_t span = (size_t)(p.rows - 1) * p.stride + p.len;
    float *dev = t->d.w ? (other ? other : store_dev(t, p.store)) + p.off : nullptr;
    std::vector<float> staged(dev ? span : 0);
    float *h = dev ? staged.data() : t->host[p.store].data() + p.off;
    if (dev && (!write || p.rows > 1)) {        // (a strided write keeps what lies between its rows)
        RPN_HIP_CHECK(hipMemcpyAsync(h, dev, span * sizeof(float), hipMemcpyDeviceToHost, s));
        RPN_HIP_CHECK(hipStreamSynchronize(s));
    }
    for (int r = 0; r < p.rows; ++r) {
        float *a = h + (size_t)r * p.stride, *b = user + (size_t)r * p.len;
        memcpy(write ? a : b, write ? b : a, p.len * sizeof(float));
    }
    if (dev && write) RPN_HIP_CHECK(hipMemcpy(dev, h, span * sizeof(float), hipMemcpyHostToDevice));
    return RPN_OK;
}

int trainer_device(rpn_head_trainer *t);

// The C ABI's parameter access in one place.  Layer `name` (bn: a BatchNorm, named by its conv, "<conv>_BN" or its Keras name) ->
// its table entries, with every refusal; then user[k] <-> the layer's k-th entry.  user: {kernel, bias} (a MobileNetV2 conv has no
// bias: NULL) or, bn, {gamma, beta, mean, var}; written only by kGet / kGrad.  kGrad reads the gradients of the last update step
// (kMaster entries only: a BatchNorm's moving statistics have none).  kSlotGet / kSlotSet: the optimizer's m (slot 0) or v (slot 1)
// of the same entries as kGrad; the state lives on the device only, which these two allocate.
enum Access { kSet, kGet, kGrad, kSlotGet, kSlotSet };

int param_access(rpn_head_trainer *t, const char *what, const char *name, bool bn, Access acc, const float *const (&user)[4], void *stream,
                 int slot = 0)
{
    RPN_REQUIRE(t && name && user[0] && (!bn || (user[1] && (acc >= kGrad || (user[2] && user[3])))), "%s: null argument", what);
    RPN_REQUIRE(acc < kSlotGet || slot == 0 || slot == 1, "%s: slot %d (0: m, 1: v)", what, slot);
    if (acc == kSet || acc == kSlotSet) t->pending_B = 0;          // new parameters: a pending forward no longer matches them
    const bool write = acc == kSet || acc == kSlotSet;
    const char *from = t->mn_from >= 0 ? mn_table()[t->mn_from].name.c_str() : (t->bb_from >= 0 ? kVgg[t->bb_from].name : "");
    const int mi = t->mn_from >= 0 ? mn_index(name, bn) : -1;
    int first, count;
    if (bn) RPN_REQUIRE(mi >= 0, "%s: '%s' is not a BatchNorm this trainer trains", what, name);
    if (mi >= 0) {
        // a MobileNetV2 conv: the kernel alone (these convs have no bias), or its BatchNorm
        RPN_REQUIRE(mi >= t->mn_from, "%s: %s'%s' is frozen (training starts at %s): it runs on the model handle", what,
                    bn || acc == kSet ? "" : "layer ", name, from);
        RPN_REQUIRE(bn || !user[1], "%s: '%s' has no bias (pass NULL)", what, name);
        first = mn_param(t, mi) + (bn ? kGamma : kKernel);
        count = bn ? (acc >= kGrad ? 2 : 4) : 1;
    } else {
        const int li = layer_index(name);
        const int bi = t->bb_from >= 0 ? vgg_index(name) : -1;
        if (acc != kSet && li < 0 && bi < 0 && t->mn_from >= 0) {     // a layer of the model below the span, or no layer of it at all
            RPN_REQUIRE(model_has_layer(t->m, name), "%s: the model has no layer named '%s'", what, name);
            return fail(RPN_ERR_INVALID, "%s: '%s' is frozen (training starts at %s): it runs on the model handle", what, name, from);
        }
        RPN_REQUIRE(user[1], "%s: null argument", what);
        RPN_REQUIRE(li >= 0 || bi >= 0,
                    acc == kSet ? "%s: '%s' is not trained (the backbone is frozen: rpn_conv, rpn_reg, rpn_cls only)"
                                : "%s: '%s' is not trained (rpn_conv, rpn_reg, rpn_cls)",
                    what, name);
        first = li >= 0 ? 2 * li : vgg_param(bi);
        count = 2;
    }
    Param *p = &t->params[first];
    if (acc == kGet || acc == kGrad) {
        for (int k = 0; k < count; ++k)
            RPN_REQUIRE(p[k].loaded, bn ? "%s: BatchNorm '%s' was never set" : "%s: layer '%s' was never set", what, name);
        RPN_REQUIRE(acc != kGrad || p->store == kMaster, "%s: layer '%s' is frozen (training starts at %s): it has no gradient", what, name,
                    from);
        RPN_REQUIRE(acc != kGrad || t->t > 0, "%s: no update step has run", what);
    }
    float *other = nullptr;
    if (acc >= kSlotGet) {
        RPN_REQUIRE(p->store == kMaster, "%s: layer '%s' is frozen (training starts at %s): it has no optimizer state", what, name, from);
        const int st = trainer_device(t);
        if (st != RPN_OK) return st;
        other = slot == 0 ? t->d.m : t->d.v;
    } else if (acc == kGrad) {
        RPN_REQUIRE(t->d.w, "%s: no update step has run", what);      // (a step count given by set_steps is no step)
        other = t->d.g;
    }
    for (int k = 0; k < count; ++k) {
        const int st = param_copy(t, p[k], const_cast<float *>(user[k]), write, other, as_stream(stream));
        if (st != RPN_OK) return st;
        if (acc == kSet) p[k].loaded = true;
    }
    return RPN_OK;
}

int trainer_check_loaded(const rpn_head_trainer *t, const char *what)
{
    for (size_t i = 0; i < t->params.size(); ++i)
        RPN_REQUIRE(t->params[i].loaded,
                    t->mn_from >= 0 && i >= kHeadParams ? "%s: layer '%s' or its BatchNorm was never set" : "%s: layer '%s' was never set", what,
                    t->params[i].layer.c_str());
    return RPN_OK;
}

// ---- device memory ------------------------------------------------------------------------------------------------------------------
// n elements for *p, recorded in the trainer's list
template <class T>
hipError_t dev_alloc(rpn_head_trainer *t, T **p, size_t n)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
    if (e == hipSuccess) t->allocs.push_back(*p);
    return e;
}

// every device buffer of the trainer freed and its pointer reset (destroy, or a failed first-step allocation)
void trainer_free(rpn_head_trainer *t)
{
    for (void *p : t->allocs) (void)hipFree(p);
    t->allocs.clear();
    t->d = TrainerDevice{};
    optim_free(&t->optdev);
}

// pixels per image of layer i's input / output
size_t mn_pin(const rpn_head_trainer *t, int i) { return (size_t)t->mn_hin[i] * t->mn_hin[i]; }
size_t mn_pout(const rpn_head_trainer *t, int i) { return (size_t)t->mn_hout[i] * t->mn_hout[i]; }

// a forward tensor the backward reads: conv i's ReLU output and its pooled form, from the input of the first trained conv upward
bool vgg_kept(const rpn_head_trainer *t, int i) { return i >= t->bb_from - 1; }
size_t vgg_act_floats(const rpn_head_trainer *t, int i) { return (size_t)t->max_batch * t->hs[i] * t->hs[i] * kVgg[i].cout; }
size_t vgg_pool_floats(const rpn_head_trainer *t, int i) { return (size_t)t->max_batch * (t->hs[i] / 2) * (t->hs[i] / 2) * kVgg[i].cout; }

size_t trainer_part_floats(const rpn_head_trainer *t)
{
    const long long P = (long long)t->max_batch * t->F * t->F;
    return std::max(std::max(head_backward_ws_floats(P, t->nc), wgrad_ws_floats(t->cin, 512)), colsum_ws_floats(P, 512));
}

// the backbone's buffers, sized by max_batch and the trained span (about 3.5 GB at batch 8, 500 x 500, from block1_conv1); the
// split-float16 backward's image and words (backbone_x3_bytes) are allocated whatever the backward precision: setting it needs no device
size_t backbone_x3_bytes(const rpn_head_trainer *t)
{
    size_t img = dgrad_x3_image_bytes(t->cin, 512);
    for (int i = std::max(1, t->bb_from + 1); i < 13; ++i) img = std::max(img, dgrad_x3_image_bytes(kVgg[i].cin, kVgg[i].cout));
    return img;
}

int backbone_device(rpn_head_trainer *t)
{
    size_t pack = 0, ping = 0, grad = 0, wpart = 0;
    RPN_HIP_CHECK(dev_alloc(t, &t->d.x3img, backbone_x3_bytes(t)));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.x3meta, 64));
    RPN_HIP_CHECK(hipMemset(t->d.x3meta, 0, 64 * sizeof(unsigned)));
    for (int i = 0; i < 13; ++i) {
        if (i > 0) pack = std::max(pack, t->ps_bb[i].floats());
        if (!vgg_kept(t, i)) ping = std::max(ping, std::max(vgg_act_floats(t, i), kVgg[i].pool ? vgg_pool_floats(t, i) : 0));
        if (i >= t->bb_from) {
            grad = std::max(grad, vgg_act_floats(t, i));
            wpart = std::max(wpart, wgrad_wide_ws_floats(t->max_batch, t->hs[i], t->hs[i], kVgg[i].cin, kVgg[i].cout));
        }
    }
    const std::vector<float> &frozen = t->host[kFrozen];
    RPN_HIP_CHECK(dev_alloc(t, &t->d.frozen, std::max<size_t>(1, frozen.size())));
    if (!frozen.empty()) RPN_HIP_CHECK(hipMemcpy(t->d.frozen, frozen.data(), frozen.size() * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.pack, pack));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.wt, (size_t)9 * 512 * 512));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.wpart, wpart));
    for (int u = 0; u < 2; ++u) {
        RPN_HIP_CHECK(dev_alloc(t, &t->d.grad[u], grad));
        if (ping) RPN_HIP_CHECK(dev_alloc(t, &t->d.ping[u], ping));
    }
    if (t->bb_from == 0) RPN_HIP_CHECK(dev_alloc(t, &t->d.img4, (size_t)t->max_batch * t->img * t->img * 4));
    for (int i = 0; i < 13; ++i) {
        if (!vgg_kept(t, i)) continue;
        RPN_HIP_CHECK(dev_alloc(t, &t->d.act[i], vgg_act_floats(t, i)));
        if (kVgg[i].pool) RPN_HIP_CHECK(dev_alloc(t, &t->d.pool[i], vgg_pool_floats(t, i)));
    }
    return RPN_OK;
}

// the span's buffers, sized by max_batch and the trained layers: per trained conv its output z (kept for the BatchNorm backward)
// and the normalised, activated tensor y (the next layer's input; the last one is d.feat)
// Every per-layer buffer is sized by that layer's own pixel count; the gradient buffers by the largest tensor they carry (mn_backward):
// d.mgr the block inputs, d.mt[0] the project outputs, d.mt[1 / 2] the expanded tensors (block_1_expand's 250 x 250 x 96 per image at
// 500 x 500) -- never less than the stride-16 span needs (F x F x 96 / 576: rpn_conv's input gradient lands in d.mt[1]).
int mn_device(rpn_head_trainer *t)
{
    const std::vector<MnConv> &tab = mn_table();
    const size_t B = (size_t)t->max_batch, PF = B * t->F * t->F;
    size_t pack = 0, wpart = 0, part = bn_part_doubles((long long)PF, 576), gr = PF * 96, t0 = PF * 96, t12 = PF * 576;
    for (int i = t->mn_from; i < kMnLayers; ++i) {
        const MnConv &l = tab[i];
        const size_t Pi = B * mn_pin(t, i), Po = B * mn_pout(t, i);
        if (l.kind == 0 || l.kind == 2) pack = std::max(pack, t->ps_mn[i].floats());
        if (l.kind == 1)
            wpart = std::max(wpart, l.stride == 2 ? dwconv3x3_s2_wgrad_ws_floats((int)B, t->mn_hin[i], t->mn_hin[i], l.cout)
                                                  : dwconv3x3_wgrad_ws_floats((long long)Po, l.cout));
        else if (l.kind == 3)
            wpart = std::max(wpart, conv3x3_s2_cin3_wgrad_ws_floats((int)B, t->mn_hin[i], t->mn_hin[i], l.cout));
        else
            wpart = std::max(wpart, conv1x1_wgrad_ws_floats((long long)Po, l.cin, l.cout));
        part = std::max(part, bn_part_doubles((long long)Po, l.cout));
        if (l.kind == 0) gr = std::max(gr, Pi * l.cin);
        if (l.kind == 2) t0 = std::max(t0, Po * l.cout);
        if (l.kind != 3) t12 = std::max(t12, std::max(Pi * l.cin, l.kind == 2 ? (size_t)0 : Po * l.cout));
        else t12 = std::max(t12, Po * l.cout);
        RPN_HIP_CHECK(dev_alloc(t, &t->d.mz[i], Po * l.cout));
        if (i < kMnLayers - 1) RPN_HIP_CHECK(dev_alloc(t, &t->d.my[i], Po * l.cout));
    }
    if (t->mn_from > 0) RPN_HIP_CHECK(dev_alloc(t, &t->d.x0, PF * tab[t->mn_from].cin));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mpack, std::max<size_t>(1, pack)));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mwpart, std::max<size_t>(1, wpart)));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mpart, part));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.bstat, t->size[kBnStep]));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.bn, t->size[kBnState]));
    RPN_HIP_CHECK(hipMemcpy(t->d.bn, t->host[kBnState].data(), t->size[kBnState] * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.wt, (size_t)9 * 512 * 576));
    for (int u = 0; u < 2; ++u) RPN_HIP_CHECK(dev_alloc(t, &t->d.mgr[u], gr));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mt[0], t0));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mt[1], t12));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.mt[2], t12));
    return RPN_OK;
}

int trainer_alloc(rpn_head_trainer *t)
{
    if (t->bb_from >= 0) {
        const int st = backbone_device(t);
        if (st != RPN_OK) return st;
    }
    if (t->mn_from >= 0) {
        const int st = mn_device(t);
        if (st != RPN_OK) return st;
    }
    const size_t P = (size_t)t->max_batch * t->F * t->F, n = t->size[kMaster];
    const struct {
        float **p;
        size_t n;
    } bufs[] = {{&t->d.w, n},         {&t->d.g, n},          {&t->d.m, n},           {&t->d.v, n},         {&t->d.pconv, t->ps_conv.floats()},
                {&t->d.phead, t->ps_head.floats()},          {&t->d.feat, P * t->cin}, {&t->d.S, P * 512},   {&t->d.reg, P * 4 * t->K},
                {&t->d.cls, P * t->K}, {&t->d.graw, P * 5 * t->K}, {&t->d.dz, P * t->nc}, {&t->d.dS, P * 512}, {&t->d.part, trainer_part_floats(t)}};
    for (const auto &b : bufs) RPN_HIP_CHECK(dev_alloc(t, b.p, b.n));
    RPN_HIP_CHECK(dev_alloc(t, &t->d.lws, losses_ws_bytes((long long)P * t->K)));
    RPN_HIP_CHECK(hipMemcpy(t->d.w, t->host[kMaster].data(), n * sizeof(float), hipMemcpyHostToDevice));
    RPN_HIP_CHECK(hipMemset(t->d.g, 0, n * sizeof(float)));       // no kernel writes the padding in front of an aligned slice
    RPN_HIP_CHECK(hipMemset(t->d.m, 0, n * sizeof(float)));
    RPN_HIP_CHECK(hipMemset(t->d.v, 0, n * sizeof(float)));
    return RPN_OK;
}

// all device buffers at the first step; d.w stays set only when every allocation and upload succeeded (a failure frees what was
// allocated, so a later step starts over instead of running on a half-built trainer)
int trainer_device(rpn_head_trainer *t)
{
    if (!have_device()) return RPN_ERR_NO_DEVICE;
    if (t->d.w) return RPN_OK;
    const int st = trainer_alloc(t);
    if (st != RPN_OK) trainer_free(t);
    return st;
}

// ---- forward and backward ---------------------------------------------------------------------------------------------------------
// a stride-1 'same' R x R conv with a single float32 output: x (B, side, side, Cin), w packed as ps -> out (B, side, side, Cout)
ConvArgs conv_same_args(const float *x, const float *w, const float *bias, float *out, int B, int side, int Cin, int Cout, int R, int act,
                        const PackedShape &ps)
{
    ConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.out = out;
    a.B = B; a.H = a.W = a.OH = a.OW = side; a.Cin = Cin; a.Cout = Cout;
    a.R = a.S = R; a.stride = 1; a.pad_t = a.pad_l = R / 2; a.ps = ps;
    a.act = act; a.act2 = ACT_LINEAR; a.split = a.ld1 = Cout; a.ld2 = 0;
    return a;
}

// The whole VGG16 forward in exact float32 from the trainer's weights (the frozen prefix included), keeping what the backward
// reads -> the block5_conv3 output (B, F, F, 512).  Weights are packed on the device at every step: the trained ones move.
hipError_t backbone_forward(rpn_head_trainer *t, const float *d_imgs, int B, hipStream_t s, const float **feat)
{
    const float *in = d_imgs;
    int ping = 0;
    auto next = [&](float *kept) -> float * {
        if (kept) return kept;
        float *p = t->d.ping[ping];
        ping ^= 1;
        return p;
    };
    if (t->bb_from == 0) {
        const hipError_t e = launch_pad_channels3to4(d_imgs, (long long)B * t->img * t->img, t->d.img4, s);
        if (e != hipSuccess) return e;
    }
    for (int i = 0; i < 13; ++i) {
        const int H = t->hs[i];
        const float *w = param_dev(t, vgg_param(i) + kKernel), *b = param_dev(t, vgg_param(i) + kBias);
        float *out = next(t->d.act[i]);
        hipError_t e;
        if (i == 0) {
            e = launch_conv_cin3(in, w, b, out, B, H, H, H, H, kVgg[0].cout, 1, 1, 1, ACT_RELU, 0, false, s);
        } else {
            pack_weights_device(t->ps_bb[i], w, t->d.pack, s);
            e = launch_conv_f32(conv_same_args(in, t->d.pack, b, out, B, H, kVgg[i].cin, kVgg[i].cout, 3, ACT_RELU, t->ps_bb[i]), s);
        }
        if (e != hipSuccess) return e;
        in = out;
        if (kVgg[i].pool) {
            float *po = next(t->d.pool[i]);
            e = launch_maxpool2x2(in, B, H, H, kVgg[i].cout, po, s);
            if (e != hipSuccess) return e;
            in = po;
        }
    }
    *feat = in;
    return hipSuccess;
}

// From dS (rpn_conv's pre-activation gradient) down to the first trained conv: dgrad (+ the ReLU mask of its input) or dgrad + the
// max-pool backward (+ the mask of the pooled conv) between layers, the weight and bias gradient of each trained conv.  add (B,F,F,cin)
// or NULL: a second stage's gradient with respect to the tap (the post-ReLU block5_conv3 output); it joins the RPN's gradient in the
// first dgrad's epilogue, before block5_conv3's ReLU mask: (dgrad + add) [feat > 0].
// With bw_precision F16X3 every dgrad and every weight gradient but block1_conv1's (Cin = 3) runs in split float16
// (train_backbone_x3_kernels.hip): one t per gradient tensor, found on the device before the two products that read it.
hipError_t backbone_backward(rpn_head_trainer *t, int B, const float *add, hipStream_t s)
{
    float *g = t->d.grad[0], *h = t->d.grad[1];
    const int F = t->hs[12];
    const bool x3 = t->bw_precision == RPN_PRECISION_F16X3;
    unsigned *meta = t->d.x3meta, *status = meta + 2;
    float *sc = reinterpret_cast<float *>(meta + 8);
    auto scale = [&](const float *dy, int H, int Cout) {
        return x3 ? launch_scale_x3(dy, (long long)B * H * H * Cout, true, meta, sc, s) : hipSuccess;
    };
    auto dgrad = [&](const float *dy, const float *w, const float *mask, const float *a, int H, int Cin, int Cout, float *dx) {
        if (!x3) return launch_conv3x3_dgrad(dy, w, mask, a, B, H, H, Cin, Cout, t->d.wt, dx, s);
        return launch_conv3x3_dgrad_x3(dy, w, mask, a, B, H, H, Cin, Cout, sc, t->d.x3img, meta + 1, sc + 2, dx, status, s);
    };
    hipError_t e = scale(t->d.dS, F, 512);
    if (e == hipSuccess) e = dgrad(t->d.dS, param_dev(t, kConvK), t->d.act[12], add, F, t->cin, 512, g);
    for (int i = 12; i >= t->bb_from && e == hipSuccess; --i) {
        const int H = t->hs[i], p = vgg_param(i);
        const float *x = i == 0 ? t->d.img4 : (kVgg[i - 1].pool ? t->d.pool[i - 1] : t->d.act[i - 1]);
        const bool wgrad_x3 = x3 && kVgg[i].cin % 4 == 0;
        if (wgrad_x3 || i > t->bb_from) e = scale(g, H, kVgg[i].cout);      // (block1_conv1 as the last layer: nobody reads the pair)
        if (e != hipSuccess) break;
        if (wgrad_x3)
            e = launch_wgrad_wide_x3(x, g, B, H, H, kVgg[i].cin, kVgg[i].cout, sc, t->d.wpart, param_grad(t, p + kKernel),
                                     param_grad(t, p + kBias), status, s);
        else
            e = launch_wgrad_wide(x, g, B, H, H, kVgg[i].cin, kVgg[i].cout, t->d.wpart, param_grad(t, p + kKernel), param_grad(t, p + kBias), s);
        if (e != hipSuccess || i == t->bb_from) break;
        if (kVgg[i - 1].pool) {
            e = dgrad(g, param_dev(t, p), nullptr, nullptr, H, kVgg[i].cin, kVgg[i].cout, h);
            if (e == hipSuccess) e = launch_maxpool2x2_backward(t->d.act[i - 1], h, B, t->hs[i - 1], t->hs[i - 1], kVgg[i - 1].cout, g, s);
        } else {
            e = dgrad(g, param_dev(t, p), t->d.act[i - 1], nullptr, H, kVgg[i].cin, kVgg[i].cout, h);
            std::swap(g, h);
        }
    }
    return e;
}

// The span's forward in exact float32 from the trainer's unfolded parameters, on top of the frozen prefix (the handle's ops up to
// mn_x0; from Conv1 there is none: the span's input is the image batch).  train: BatchNorm normalises with the batch statistics and
// updates the moving ones; else with the moving statistics (inference mode, nothing updated).  Every conv output z and every layer
// output y is kept.  -> the block_13_expand output in d.feat.
int mn_forward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, bool train, hipStream_t s)
{
    const std::vector<MnConv> &tab = mn_table();
    if (t->mn_from > 0) {
        const int e0 = model_features_at(t->m, t->mn_x0.c_str(), d_imgs, B, t->d.x0, s);
        if (e0 != RPN_OK) return e0;
    }
    t->d.my[kMnLayers - 1] = t->d.feat;
    for (int i = t->mn_from; i < kMnLayers; ++i) {
        const MnConv &l = tab[i];
        const int H = t->mn_hin[i], F = t->mn_hout[i], p = mn_param(t, i);
        const long long P = (long long)B * F * F;
        const float *in = i == t->mn_from ? (i == 0 ? d_imgs : t->d.x0) : t->d.my[i - 1];
        const float *w = param_dev(t, p + kKernel);
        hipError_t e;
        if (l.kind == 1) {
            const int pad = l.stride == 2 ? H % 2 : 1;
            e = launch_dwconv3x3(in, B, H, H, l.cout, w, nullptr, l.stride, pad, pad, F, F, ACT_LINEAR, t->d.mz[i], s);
        } else if (l.kind == 3) {
            e = launch_conv_cin3(in, w, nullptr, t->d.mz[i], B, H, H, F, F, l.cout, 2, H % 2, H % 2, ACT_LINEAR, 0, false, s);
        } else {
            pack_weights_device(t->ps_mn[i], w, t->d.mpack, s);
            e = launch_conv_f32(conv_same_args(in, t->d.mpack, nullptr, t->d.mz[i], B, F, l.cin, l.cout, 1, ACT_LINEAR, t->ps_mn[i]), s);
        }
        float *mean = param_dev(t, p + kStats), *var = mean + l.cout, *rstd = var + l.cout;
        float *mmean = param_dev(t, p + kMean), *mvar = param_dev(t, p + kVar);
        if (e == hipSuccess) {
            if (train) {
                e = launch_bn_train_stats(t->d.mz[i], P, l.cout, kMnBnEps, kMnBnMomentum, t->d.mpart, mean, var, rstd, mmean, mvar, s);
            } else {                            // (mean | var are adjacent in both stores)
                e = hipMemcpyAsync(mean, mmean, (size_t)2 * l.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
                if (e == hipSuccess) e = launch_bn_rstd(mvar, l.cout, kMnBnEps, rstd, s);
            }
        }
        const float *res = (l.kind == 2 && l.res) ? (i - 2 == t->mn_from ? t->d.x0 : t->d.my[i - 3]) : nullptr;
        if (e == hipSuccess)
            e = launch_bn_apply(t->d.mz[i], P, l.cout, mean, rstd, param_dev(t, p + kGamma), param_dev(t, p + kBeta), l.kind != 2, res,
                                t->d.my[i], s);
        if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s: %s", what, l.name.c_str(), hipGetErrorString(e));
    }
    return RPN_OK;
}

// From dS (rpn_conv's pre-activation gradient) down to the first trained layer.  g: the gradient of the current layer's output.  A
// residual block's output gradient stays in d.mgr[a] until the block's expand dgrad adds it to what that conv sends to the block's
// input (the dgrad's epilogue: no atomics, no extra pass).  add (B,F,F,cin) or NULL: a second stage's gradient with respect to the
// tap (block_13_expand after its ReLU6); it joins the RPN's gradient in the first dgrad's epilogue, and the BatchNorm backward that
// follows applies the ReLU6 mask to the sum.
hipError_t mn_backward(rpn_head_trainer *t, const float *d_imgs, int B, const float *add, hipStream_t s)
{
    const std::vector<MnConv> &tab = mn_table();
    float *g = t->d.mt[1];
    const float *gres = nullptr;
    int a = 1;
    hipError_t e = launch_conv3x3_dgrad(t->d.dS, param_dev(t, kConvK), nullptr, add, B, t->F, t->F, t->cin, 512, t->d.wt, g, s);
    for (int i = kMnLayers - 1; i >= t->mn_from && e == hipSuccess; --i) {
        const MnConv &l = tab[i];
        const int H = t->mn_hin[i], F = t->mn_hout[i], p = mn_param(t, i);
        const long long P = (long long)B * F * F;
        const float *in = i == t->mn_from ? (i == 0 ? d_imgs : t->d.x0) : t->d.my[i - 1];
        const float *w = param_dev(t, p + kKernel);
        float *dw = param_grad(t, p + kKernel);
        const float *mean = param_dev(t, p + kStats), *rstd = mean + 2 * l.cout;
        float *dz = g;
        if (l.kind == 2) {
            if (l.res) gres = g;
            dz = t->d.mt[0];
        }
        e = launch_bn_backward(t->d.mz[i], g, P, l.cout, mean, rstd, param_dev(t, p + kGamma), param_dev(t, p + kBeta), l.kind != 2,
                               t->d.mpart, param_grad(t, p + kGamma), param_grad(t, p + kBeta), dz, s);
        if (e != hipSuccess) break;
        if (l.kind == 3) {                      // the stem: its input is the image, so there is no data gradient
            e = launch_conv3x3_s2_cin3_wgrad(in, dz, B, H, H, l.cout, t->d.mwpart, dw, s);
            break;
        }
        if (l.kind == 1) {
            float *dx = dz == t->d.mt[1] ? t->d.mt[2] : t->d.mt[1];
            if (l.stride == 2) {
                e = launch_dwconv3x3_s2_wgrad(in, dz, B, H, H, l.cout, t->d.mwpart, dw, s);
                if (e == hipSuccess) e = launch_dwconv3x3_s2_dgrad(dz, w, B, H, H, l.cout, dx, s);
            } else {
                e = launch_dwconv3x3_wgrad(in, dz, B, F, F, l.cout, t->d.mwpart, dw, s);
                if (e == hipSuccess) e = launch_dwconv3x3_dgrad(dz, w, B, F, F, l.cout, dx, s);
            }
            g = dx;
            continue;
        }
        e = launch_conv1x1_wgrad(in, dz, P, l.cin, l.cout, t->d.mwpart, dw, s);
        if (e != hipSuccess || i == t->mn_from) break;
        if (l.kind == 2) {
            g = t->d.mt[1];
            e = launch_conv1x1_dgrad(dz, w, nullptr, P, l.cin, l.cout, g, s);
        } else {
            float *dx = t->d.mgr[a ^ 1];
            e = launch_conv1x1_dgrad(dz, w, gres, P, l.cin, l.cout, dx, s);
            a ^= 1;
            g = dx;
            gres = nullptr;
        }
    }
    return e;
}

// the host copies of the stores, zeroed, once the table is complete
void trainer_host_stores(rpn_head_trainer *t)
{
    for (int s = 0; s < kBnStep; ++s) t->host[s].assign(t->size[s], 0.0f);
}

// The decayed elements of kMaster, as sorted disjoint [begin, end) pairs: every trained kernel -- rpn_conv's, rows 0 .. 511 of the fused
// head matrix (the rpn_reg and rpn_cls columns together; row 512 is its bias), each trained backbone conv's -- and nothing else: no
// bias, gamma or beta and no alignment gap.  Host arithmetic on the table.
std::vector<long long> trainer_decay_ranges(const rpn_head_trainer *t)
{
    std::vector<int> idx = {kConvK, kHeadK, kClsK};
    for (int i = std::max(t->bb_from, 0); t->bb_from >= 0 && i < 13; ++i) idx.push_back(vgg_param(i) + kKernel);
    for (int i = std::max(t->mn_from, 0); t->mn_from >= 0 && i < kMnLayers; ++i) idx.push_back(mn_param(t, i) + kKernel);
    std::vector<std::pair<long long, long long>> spans;
    for (int i : idx) {
        const Param &p = t->params[i];
        spans.push_back({(long long)p.off, (long long)(p.off + (size_t)(p.rows - 1) * p.stride + p.len)});
    }
    std::sort(spans.begin(), spans.end());
    std::vector<long long> out;
    for (const auto &sp : spans) {
        if (!out.empty() && sp.first <= out.back()) out.back() = std::max(out.back(), sp.second);
        else out.push_back(sp.first), out.push_back(sp.second);
    }
    return out;
}

}  // namespace

// ---- C ABI: creation ----------------------------------------------------------------------------------------------------------------
extern "C" int rpn_head_trainer_create(rpn_model *m, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_head_trainer_create: null argument");
    int cin, F, K, mb;
    model_train_dims(m, &cin, &F, &K, &mb);
    RPN_REQUIRE(cin % 4 == 0 && 5 * K <= 64 && K >= 1, "rpn_head_trainer_create: unsupported head (Cin %d, K %d)", cin, K);
    rpn_head_trainer *t = new rpn_head_trainer();
    t->m = m; t->cin = cin; t->F = F; t->K = K; t->max_batch = mb; t->nc = 5 * K;
    const int nc = t->nc;
    param_append(t, "rpn_conv", kMaster, (size_t)9 * cin * 512);
    param_append(t, "rpn_conv", kMaster, 512);
    const size_t hk = t->size[kMaster], hb = hk + (size_t)512 * nc;     // the fused head matrix (512, nc) and its bias (nc)
    t->params.push_back({"rpn_reg", kMaster, hk, 512, 4 * K, nc, false});
    t->params.push_back({"rpn_reg", kMaster, hb, 1, 4 * K, 4 * K, false});
    t->params.push_back({"rpn_cls", kMaster, hk + 4 * K, 512, K, nc, false});
    t->params.push_back({"rpn_cls", kMaster, hb + 4 * K, 1, K, K, false});
    t->size[kMaster] = hb + nc;
    trainer_host_stores(t);
    t->ps_conv = packed_shape(3, 3, cin, 512);
    t->ps_head = packed_shape(1, 1, 512, nc);
    *out = t;
    return RPN_OK;
}

// the MobileNetV2 trainer from layer `from` of mn_table() up: an expand conv of the stride-16 span, or 0 (Conv1: the whole model)
static int mn_trainer_create(rpn_model *m, int from, int img, const char *what, rpn_head_trainer **out)
{
    const std::vector<MnConv> &tab = mn_table();
    rpn_head_trainer *t = nullptr;
    const int st = rpn_head_trainer_create(m, &t);
    if (st != RPN_OK) return st;
    for (int i = 0, h = img; i < kMnLayers; ++i) {          // each layer's own resolution, from the image down
        t->mn_hin[i] = h;
        if (tab[i].stride == 2) {
            int pad;
            mn_s2_geom(h, &pad, &h);
        }
        t->mn_hout[i] = h;
    }
    bool ok = t->cin == 576 && t->mn_hout[kMnLayers - 1] == t->F && t->F >= 1;
    if (from > 0) {
        t->mn_x0 = tab[from - 1].name;
        int h = 0, w = 0, c = 0;
        ok = ok && model_tensor_shape(m, t->mn_x0.c_str(), &h, &w, &c) == RPN_OK && h == t->F && w == t->F && c == tab[from].cin;
    } else {
        ok = ok && (long long)t->max_batch * t->mn_hout[0] * t->mn_hout[0] <= (1ll << 21);       // the 1x1 GEMMs' row count (gemm_ok)
    }
    if (!ok) {
        rpn_head_trainer_destroy(t);
        return fail(RPN_ERR_UNSUPPORTED, "%s: unexpected MobileNetV2 graph below '%s'", what, tab[from].name.c_str());
    }
    t->img = img;
    t->mn_from = from;
    for (int i = from; i < kMnLayers; ++i) {                // kMnRoles entries per layer, in the order of Role
        t->size[kMaster] = (t->size[kMaster] + 3) & ~(size_t)3;
        param_append(t, tab[i].name, kMaster, mn_kernel_floats(i));
        param_append(t, tab[i].name, kMaster, tab[i].cout);
        param_append(t, tab[i].name, kMaster, tab[i].cout);
        param_append(t, tab[i].name, kBnState, tab[i].cout);
        param_append(t, tab[i].name, kBnState, tab[i].cout);
        param_append(t, tab[i].name, kBnStep, (size_t)3 * tab[i].cout);
        if (tab[i].kind == 0 || tab[i].kind == 2) t->ps_mn[i] = packed_shape(1, 1, tab[i].cin, tab[i].cout);
    }
    trainer_host_stores(t);
    *out = t;
    return RPN_OK;
}

extern "C" int rpn_model_trainer_create_full(rpn_model *m, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_model_trainer_create_full: null argument");
    int backbone, img;
    model_train_backbone(m, &backbone, &img);
    if (backbone == RPN_BACKBONE_MOBILENET_V2) return mn_trainer_create(m, 0, img, "rpn_model_trainer_create_full", out);
    RPN_REQUIRE(backbone == RPN_BACKBONE_VGG16, "rpn_model_trainer_create_full: unknown backbone %d", backbone);
    return rpn_model_trainer_create(m, kVgg[0].name, out);
}

extern "C" int rpn_model_trainer_create(rpn_model *m, const char *train_from, rpn_head_trainer **out)
{
    RPN_REQUIRE(m && out, "rpn_model_trainer_create: null argument");
    if (!train_from) return rpn_head_trainer_create(m, out);
    int backbone, img;
    model_train_backbone(m, &backbone, &img);
    if (backbone == RPN_BACKBONE_MOBILENET_V2) {
        const std::vector<MnConv> &tab = mn_table();
        const int from = mn_index(train_from);
        RPN_REQUIRE(from >= kMnSpan && tab[from].kind == 0,
                    "rpn_model_trainer_create: '%s' does not start a trainable span of MobileNetV2: accepted are block_7_expand .. "
                    "block_12_expand and block_13_expand (that layer and every layer above it train with the head); otherwise this "
                    "backbone trains its head only -- the layer is a VGG16 conv, is not the first layer of a block, or lies below "
                    "block_7_expand (rpn_model_trainer_create_full trains the whole model)", train_from);
        return mn_trainer_create(m, from, img, "rpn_model_trainer_create", out);
    }
    RPN_REQUIRE(backbone == RPN_BACKBONE_VGG16, "rpn_model_trainer_create: unknown backbone %d", backbone);
    const int from = vgg_index(train_from);
    RPN_REQUIRE(from >= 0, "rpn_model_trainer_create: '%s' is not a VGG16 conv (block1_conv1 .. block5_conv3)", train_from);
    rpn_head_trainer *t = nullptr;
    int st = rpn_head_trainer_create(m, &t);
    if (st != RPN_OK) return st;
    for (int i = 0, h = img; i < 13; ++i) {
        t->hs[i] = h;
        if (kVgg[i].pool) h /= 2;
    }
    if (t->cin != 512 || t->F != t->hs[12] || t->F < 1) {
        st = fail(RPN_ERR_UNSUPPORTED, "rpn_model_trainer_create: unexpected VGG16 graph (features %d, F %d)", t->cin, t->F);
        rpn_head_trainer_destroy(t);
        return st;
    }
    t->bb_from = from;
    t->img = img;
    for (int i = 0; i < 13; ++i) {              // all 13: the trained convs follow the head in kMaster, the others fill kFrozen
        param_append(t, kVgg[i].name, i >= from ? kMaster : kFrozen, (size_t)9 * kVgg[i].cin * kVgg[i].cout);
        param_append(t, kVgg[i].name, i >= from ? kMaster : kFrozen, kVgg[i].cout);
        if (i > 0) t->ps_bb[i] = packed_shape(3, 3, kVgg[i].cin, kVgg[i].cout);
    }
    trainer_host_stores(t);
    *out = t;
    return RPN_OK;
}

extern "C" void rpn_head_trainer_destroy(rpn_head_trainer *t)
{
    if (!t) return;
    trainer_free(t);
    delete t;
}

// ---- C ABI: parameters (HOST arrays; param_access).  A BatchNorm is named by its conv or by its own layer ("<conv>_BN") ---------------
extern "C" int rpn_head_trainer_set_layer(rpn_head_trainer *t, const char *name, const float *kernel, const float *bias)
{
    return param_access(t, "rpn_head_trainer_set_layer", name, false, kSet, {kernel, bias}, nullptr);
}

extern "C" int rpn_head_trainer_get_layer(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_layer", name, false, kGet, {kernel, bias}, stream);
}

extern "C" int rpn_head_trainer_get_gradient(rpn_head_trainer *t, const char *name, float *kernel, float *bias, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_gradient", name, false, kGrad, {kernel, bias}, stream);
}

extern "C" int rpn_head_trainer_set_bn(rpn_head_trainer *t, const char *name, const float *gamma, const float *beta, const float *mean,
                                       const float *var)
{
    return param_access(t, "rpn_head_trainer_set_bn", name, true, kSet, {gamma, beta, mean, var}, nullptr);
}

extern "C" int rpn_head_trainer_get_bn(rpn_head_trainer *t, const char *name, float *gamma, float *beta, float *mean, float *var, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_bn", name, true, kGet, {gamma, beta, mean, var}, stream);
}

extern "C" int rpn_head_trainer_get_bn_gradient(rpn_head_trainer *t, const char *name, float *dgamma, float *dbeta, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_bn_gradient", name, true, kGrad, {dgamma, dbeta}, stream);
}

// ---- a step in two halves: forward + losses (+ the loss gradients), then head backward, backbone backward and Adam ------------------
// `what` names the public entry in the messages.  rpn_head_trainer_step = both halves back to back: the same launches in the same
// order on the same buffers as the closed call it was.
static int trainer_check_forward(const rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_bbox_deltas,
                                 const float *d_bbox_labels, const float *d_losses)
{
    RPN_REQUIRE(t && d_imgs && d_bbox_deltas && d_bbox_labels && d_losses, "%s: null argument", what);
    RPN_REQUIRE(B >= 1 && B <= t->max_batch, "%s: batch %d outside [1, %d]", what, B, t->max_batch);
    return RPN_OK;
}

static int trainer_check_adam(const rpn_head_trainer *t, const char *what, float lr, float beta_1, float beta_2, float epsilon)
{
    if (t->opt.kind == RPN_OPT_SGD) {           // beta_1, beta_2 and epsilon are ignored
        RPN_REQUIRE(std::isfinite(lr) && lr >= 0.0f, "%s: bad SGD learning rate", what);
        return RPN_OK;
    }
    RPN_REQUIRE(std::isfinite(lr) && lr >= 0.0f && beta_1 >= 0.0f && beta_1 < 1.0f && beta_2 >= 0.0f && beta_2 < 1.0f &&
                    std::isfinite(epsilon) && epsilon >= 0.0f,
                "%s: bad Adam hyper-parameters", what);
    return RPN_OK;
}

// the arguments are checked by the caller
static int trainer_forward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_bbox_deltas,
                           const float *d_bbox_labels, int train, float *d_losses, void *stream)
{
    t->pending_B = 0;                           // whatever happens below, the buffers of an earlier forward are being overwritten:
    t->pending_imgs = nullptr;                  // nothing is pending, and feature / outputs have nothing to return until this one is done
    t->last_B = 0;
    t->d_tap = nullptr;
    const int st = trainer_device(t);
    if (st != RPN_OK) return st;
    hipStream_t s = as_stream(stream);
    const int F = t->F, K = t->K, nc = t->nc;
    const long long P = (long long)B * F * F;
    const float *feat = t->d.feat;
    if (t->bb_from >= 0) {
        // a trained backbone: the whole VGG16 in exact float32 from the trainer's weights
        const hipError_t eb = backbone_forward(t, d_imgs, B, s, &feat);
        if (eb != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: backbone: %s", what, hipGetErrorString(eb));
    } else if (t->mn_from >= 0) {
        // a trained MobileNetV2 span: BatchNorm in training mode on an update step, in inference mode on an evaluation
        const int e0 = mn_forward(t, what, d_imgs, B, train != 0, s);
        if (e0 != RPN_OK) return e0;
    } else {
        const int e0 = model_features(t->m, d_imgs, B, t->d.feat, s);
        if (e0 != RPN_OK) return e0;
    }
    // head forward in exact float32 from the master weights
    pack_weights_device(t->ps_conv, param_dev(t, kConvK), t->d.pconv, s);
    pack_weights_device(t->ps_head, param_dev(t, kHeadK), t->d.phead, s);
    hipError_t e = launch_conv_f32(conv_same_args(feat, t->d.pconv, param_dev(t, kConvB), t->d.S, B, F, t->cin, 512, 3, ACT_RELU, t->ps_conv), s);
    if (e == hipSuccess) {
        // the fused head: one conv, the rpn_reg columns linear into d.reg, the rpn_cls columns through the sigmoid into d.cls
        ConvArgs h = conv_same_args(t->d.S, t->d.phead, param_dev(t, kHeadB), t->d.reg, B, F, 512, nc, 1, ACT_LINEAR, t->ps_head);
        h.split = h.ld1 = 4 * K;
        h.out2 = t->d.cls; h.ld2 = K; h.act2 = ACT_SIGMOID;
        e = launch_conv_f32(h, s);
    }
    float *graw_reg = t->d.graw, *graw_cls = t->d.graw + P * 4 * K;
    const long long n = P * K;                  // (B, A) with A = F F K
    if (e == hipSuccess)
        e = launch_losses(d_bbox_deltas, t->d.reg, d_bbox_labels, t->d.cls, n, train ? graw_reg : nullptr, train ? graw_cls : nullptr,
                          d_losses, 1, t->d.lws, s);
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
    t->last_B = B;
    t->d_tap = feat;
    if (train) {
        t->pending_B = B;
        t->pending_imgs = d_imgs;
    }
    return RPN_OK;
}

// the pending forward's B and d_imgs and the Adam parameters are checked by the caller
static int trainer_backward(rpn_head_trainer *t, const char *what, const float *d_imgs, int B, const float *d_feature_grad, float lr,
                            float beta_1, float beta_2, float epsilon, void *stream)
{
    hipStream_t s = as_stream(stream);
    const int F = t->F, K = t->K;
    const long long P = (long long)B * F * F;
    const long long n = P * K;
    const float *graw_reg = t->d.graw, *graw_cls = t->d.graw + P * 4 * K;
    t->pending_B = 0;                           // consumed, whatever happens below
    t->pending_imgs = nullptr;
    bool supported;
    // (the head's kernel and bias gradients are adjacent: 513 rows of nc)
    hipError_t e = launch_head_backward(graw_reg, graw_cls, t->d.cls, losses_scale(t->d.lws, n), t->d.S, param_dev(t, kHeadK), P, K, t->d.dz,
                                        t->d.part, param_grad(t, kHeadK), t->d.dS, &supported, s);
    if (!supported) return fail(RPN_ERR_UNSUPPORTED, "%s: %d anchors per position", what, K);
    if (e == hipSuccess) e = launch_wgrad(t->d_tap, t->d.dS, B, F, F, t->cin, 512, t->d.part, param_grad(t, kConvK), s);
    if (e == hipSuccess) e = launch_colsum(t->d.dS, P, 512, t->d.part, param_grad(t, kConvB), s);
    if (e == hipSuccess && t->bb_from >= 0) e = backbone_backward(t, B, d_feature_grad, s);
    if (e == hipSuccess && t->mn_from >= 0) e = mn_backward(t, d_imgs, B, d_feature_grad, s);
    if (e == hipSuccess && !t->opt.is_default()) {          // another rule, a decay or a clip norm: the norm pass (if any) + one launch
        ++t->t;
        const std::vector<long long> ranges = t->optdev.buf ? std::vector<long long>() : trainer_decay_ranges(t);
        return optim_step(what, t->opt, &t->optdev, ranges.data(), (int)(ranges.size() / 2), t->d.w, t->d.g, t->d.m, t->d.v,
                          (long long)t->size[kMaster], t->t, lr, beta_1, beta_2, epsilon, s);
    }
    if (e == hipSuccess) {
        ++t->t;
        e = launch_adam(t->d.w, t->d.g, t->d.m, t->d.v, (long long)t->size[kMaster], t->t, lr, beta_1, beta_2, epsilon, s);
    }
    if (e != hipSuccess) return fail(RPN_ERR_NO_DEVICE, "%s: %s", what, hipGetErrorString(e));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_step(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                                     const float *d_bbox_labels, int update, float lr, float beta_1, float beta_2, float epsilon,
                                     float *d_losses, void *stream)
{
    const char *what = "rpn_head_trainer_step";
    int st = trainer_check_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, d_losses);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(update == 0 || update == 1, "rpn_head_trainer_step: update must be 0 or 1");
    if (update && (st = trainer_check_adam(t, what, lr, beta_1, beta_2, epsilon)) != RPN_OK) return st;
    if ((st = trainer_check_loaded(t, what)) != RPN_OK) return st;
    st = trainer_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, update, d_losses, stream);
    if (st != RPN_OK || !update) return st;
    return trainer_backward(t, what, d_imgs, B, nullptr, lr, beta_1, beta_2, epsilon, stream);
}

extern "C" int rpn_head_trainer_forward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_bbox_deltas,
                                        const float *d_bbox_labels, int train, float *d_losses, void *stream)
{
    const char *what = "rpn_head_trainer_forward";
    int st = trainer_check_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, d_losses);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(train == 0 || train == 1, "rpn_head_trainer_forward: train must be 0 or 1");
    if ((st = trainer_check_loaded(t, what)) != RPN_OK) return st;
    return trainer_forward(t, what, d_imgs, B, d_bbox_deltas, d_bbox_labels, train, d_losses, stream);
}

extern "C" int rpn_head_trainer_feature(rpn_head_trainer *t, float *d_out, int B, void *stream)
{
    RPN_REQUIRE(t && d_out, "rpn_head_trainer_feature: null argument");
    RPN_REQUIRE(B >= 1 && B == t->last_B && t->d_tap, "rpn_head_trainer_feature: batch %d, the last forward ran %d images", B, t->last_B);
    RPN_REQUIRE_DEVICE();
    RPN_HIP_CHECK(hipMemcpyAsync(d_out, t->d_tap, (size_t)B * t->F * t->F * t->cin * sizeof(float), hipMemcpyDeviceToDevice,
                                 as_stream(stream)));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_backward(rpn_head_trainer *t, const float *d_imgs, int B, const float *d_feature_grad, float lr,
                                         float beta_1, float beta_2, float epsilon, void *stream)
{
    const char *what = "rpn_head_trainer_backward";
    RPN_REQUIRE(t, "rpn_head_trainer_backward: null argument");
    RPN_REQUIRE(!d_feature_grad || t->bb_from >= 0 || t->mn_from >= 0,
                "rpn_head_trainer_backward: d_feature_grad given to a trainer with a frozen backbone: nothing below the feature tap trains "
                "(create the trainer with rpn_model_trainer_create and a train_from layer)");
    RPN_REQUIRE(d_imgs, "rpn_head_trainer_backward: null argument");
    const int st = trainer_check_adam(t, what, lr, beta_1, beta_2, epsilon);
    if (st != RPN_OK) return st;
    RPN_REQUIRE(t->pending_B > 0, "rpn_head_trainer_backward: no pending rpn_head_trainer_forward with train = 1 on this trainer");
    RPN_REQUIRE(B == t->pending_B, "rpn_head_trainer_backward: batch %d, the pending forward ran %d images", B, t->pending_B);
    RPN_REQUIRE(d_imgs == t->pending_imgs, "rpn_head_trainer_backward: d_imgs is not the pending forward's image batch");
    RPN_REQUIRE(((uintptr_t)d_feature_grad & 3) == 0, "rpn_head_trainer_backward: d_feature_grad must be 4-byte aligned");
    return trainer_backward(t, what, d_imgs, B, d_feature_grad, lr, beta_1, beta_2, epsilon, stream);
}

extern "C" long long rpn_head_trainer_steps(const rpn_head_trainer *t) { return t ? t->t : -1; }

// ---- C ABI: the update rule and the optimizer's state (include/rpn_hip.h, "Optimizers") -------------------------------------------------
extern "C" int rpn_head_trainer_set_optimizer(rpn_head_trainer *t, int kind, float momentum, int nesterov, float weight_decay,
                                              float global_clipnorm)
{
    const char *who = "rpn_head_trainer_set_optimizer";
    RPN_REQUIRE(t, "%s: null argument", who);
    const int st = optim_check_config(who, kind, momentum, nesterov, weight_decay, global_clipnorm);
    if (st != RPN_OK) return st;
    t->pending_B = 0;
    t->pending_imgs = nullptr;
    if (kind != t->opt.kind) {                  // the other rule's m and v mean nothing to this one
        if (t->d.w) {
            RPN_HIP_CHECK(hipMemset(t->d.m, 0, t->size[kMaster] * sizeof(float)));
            RPN_HIP_CHECK(hipMemset(t->d.v, 0, t->size[kMaster] * sizeof(float)));
        }
        t->t = 0;
    }
    t->opt.kind = kind, t->opt.momentum = momentum, t->opt.nesterov = nesterov, t->opt.weight_decay = weight_decay;
    t->opt.clipnorm = global_clipnorm;
    t->optdev.stepped = false;
    return RPN_OK;
}

extern "C" int rpn_head_trainer_grad_norm(rpn_head_trainer *t, double *norm, float *scale, void *stream)
{
    RPN_REQUIRE(t, "rpn_head_trainer_grad_norm: null argument");
    return optim_grad_norm("rpn_head_trainer_grad_norm", t->opt, t->optdev, norm, scale, as_stream(stream));
}

extern "C" int rpn_head_trainer_decay_ranges(const rpn_head_trainer *t, long long *ranges, int cap)
{
    if (!t) return -1;
    const std::vector<long long> r = trainer_decay_ranges(t);
    const int n = (int)(r.size() / 2);
    for (int i = 0; ranges && i < std::min(n, cap); ++i) ranges[2 * i] = r[2 * i], ranges[2 * i + 1] = r[2 * i + 1];
    return n;
}

extern "C" int rpn_head_trainer_get_slot(rpn_head_trainer *t, const char *name, int slot, float *kernel, float *bias, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_slot", name, false, kSlotGet, {kernel, bias}, stream, slot);
}

extern "C" int rpn_head_trainer_set_slot(rpn_head_trainer *t, const char *name, int slot, const float *kernel, const float *bias)
{
    return param_access(t, "rpn_head_trainer_set_slot", name, false, kSlotSet, {kernel, bias}, nullptr, slot);
}

extern "C" int rpn_head_trainer_get_bn_slot(rpn_head_trainer *t, const char *name, int slot, float *gamma, float *beta, void *stream)
{
    return param_access(t, "rpn_head_trainer_get_bn_slot", name, true, kSlotGet, {gamma, beta}, stream, slot);
}

extern "C" int rpn_head_trainer_set_bn_slot(rpn_head_trainer *t, const char *name, int slot, const float *gamma, const float *beta)
{
    return param_access(t, "rpn_head_trainer_set_bn_slot", name, true, kSlotSet, {gamma, beta}, nullptr, slot);
}

extern "C" int rpn_head_trainer_set_steps(rpn_head_trainer *t, long long steps)
{
    RPN_REQUIRE(t && steps >= 0, "rpn_head_trainer_set_steps: null trainer or steps = %lld < 0", steps);
    t->pending_B = 0;
    t->pending_imgs = nullptr;
    t->t = steps;
    return RPN_OK;
}

// ---- C ABI: the arithmetic of the backbone's backward products ---------------------------------------------------------------------------
extern "C" int rpn_head_trainer_set_backward_precision(rpn_head_trainer *t, int precision)
{
    const char *who = "rpn_head_trainer_set_backward_precision";
    RPN_REQUIRE(t, "%s: null argument", who);
    RPN_REQUIRE(precision >= RPN_PRECISION_F32 && precision <= RPN_PRECISION_F32W, "%s: unknown precision %d", who, precision);
    if (precision == RPN_PRECISION_BF16X3 || precision == RPN_PRECISION_F32W)
        return fail(RPN_ERR_UNSUPPORTED, "%s: the backward runs in RPN_PRECISION_F32 or RPN_PRECISION_F16X3 only", who);
    if (precision == RPN_PRECISION_F16X3 && t->bb_from < 0)
        return fail(RPN_ERR_UNSUPPORTED, t->mn_from >= 0 ? "%s: the MobileNetV2 backward has no split-float16 kernels (VGG16 only)"
                                                         : "%s: this trainer trains the head only: there is no backbone backward to run in split float16",
                    who);
    t->bw_precision = precision;
    return RPN_OK;
}

extern "C" int rpn_head_trainer_backward_precision(const rpn_head_trainer *t) { return t ? t->bw_precision : RPN_PRECISION_F32; }

extern "C" size_t rpn_head_trainer_backward_x3_bytes(const rpn_head_trainer *t)
{
    return t && t->bb_from >= 0 ? backbone_x3_bytes(t) + 64 * sizeof(unsigned) : 0;
}

extern "C" int rpn_head_trainer_status(rpn_head_trainer *t, unsigned *flags, int reset, void *stream)
{
    RPN_REQUIRE(t && flags, "rpn_head_trainer_status: null argument");
    *flags = 0;
    if (!t->d.x3meta) return RPN_OK;          // no VGG16 span, or the trainer has not touched the device yet
    const hipStream_t s = as_stream(stream);
    RPN_HIP_CHECK(hipMemcpyAsync(flags, t->d.x3meta + 2, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    if (reset) RPN_HIP_CHECK(hipMemsetAsync(t->d.x3meta + 2, 0, sizeof(unsigned), s));
    RPN_HIP_CHECK(hipStreamSynchronize(s));
    return RPN_OK;
}

extern "C" int rpn_head_trainer_outputs(rpn_head_trainer *t, float *d_reg, float *d_cls, int B, void *stream)
{
    RPN_REQUIRE(t && d_reg && d_cls, "rpn_head_trainer_outputs: null argument");
    RPN_REQUIRE(B >= 1 && B == t->last_B, "rpn_head_trainer_outputs: batch %d, the last step ran %d images", B, t->last_B);
    RPN_REQUIRE_DEVICE();
    const size_t P = (size_t)B * t->F * t->F;
    RPN_HIP_CHECK(hipMemcpyAsync(d_reg, t->d.reg, P * 4 * t->K * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    RPN_HIP_CHECK(hipMemcpyAsync(d_cls, t->d.cls, P * t->K * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
    return RPN_OK;
}
