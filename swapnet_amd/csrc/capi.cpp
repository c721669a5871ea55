// swapnet_amd -- extern "C" boundary (include/swapnet_hip.h).  Plain pointers and sizes only.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/swapnet_hip.h"
#include <cstdlib>

#include "engine.h"

using namespace swn;

// The context is shared-owned by its handle and by every model / pipeline created in it: destroying the handles in
// any order (interpreter shutdown) is safe, and a model's destructor can always hand its buffers back.
struct CtxBox {
  std::unique_ptr<Ctx> c;
  void* owned_stream = nullptr;
  ~CtxBox() { c.reset(); if (owned_stream) stream_destroy(owned_stream); }
};
struct swn_ctx {
  std::shared_ptr<CtxBox> box;
  Ctx* c = nullptr;
};
struct swn_model {
  std::shared_ptr<CtxBox> keep;     // declared first: released after the model
  std::shared_ptr<Model> sharer;    // the model whose arenas this one uses (swn_model_create_shared): outlives it
  std::shared_ptr<Model> m;
  // what it was created with (a sharing model is created like its sharer, at another batch size)
  int kind = 0, is_train = 1, num_roi = 12, body_channels = 3, cloth_channels = 19, patchgan_layers = 3, patchgan_norm = 0;
  int netG = 0;                     // texture models: --netG (0 swapnet, 1 unet_128)
  float dropout = 0.5f;
};
struct swn_pipeline {
  std::shared_ptr<CtxBox> keep;
  std::unique_ptr<Pipeline> p;
};

static thread_local std::string g_err;

template <typename F>
static int guard(F f) {
  try {
    f();
    return 0;
  } catch (const Error& e) {
    g_err = e.what();
    return e.code ? e.code : 1;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  } catch (...) {
    g_err = "unknown error";
    return 1;
  }
}
#define REQUIRE(cond, msg) \
  do { if (!(cond)) throw Error(1, msg); } while (0)

extern "C" {

int swn_abi_version(void) { return 9; }
const char* swn_last_error(void) { return g_err.c_str(); }
int swn_is_device_build(void) { return is_device_build(); }

int swn_ctx_create(int device, void* hip_stream, int create_stream, size_t workspace_bytes, swn_ctx** out) {
  return guard([&] {
    REQUIRE(out, "swn_ctx_create: out is NULL");
    auto h = std::make_unique<swn_ctx>();
    h->box = std::make_shared<CtxBox>();
    void* st = hip_stream;
    if (create_stream) { st = stream_create(device); h->box->owned_stream = st; }
    else device_check(device);
    if (workspace_bytes < (size_t)64 << 20) workspace_bytes = (size_t)64 << 20;
    h->box->c = std::make_unique<Ctx>(st, workspace_bytes);
    h->c = h->box->c.get();
    h->c->device_index = device;
    if (env_on(getenv("SWN_OVERLAP"))) h->c->enable_side(device);
    *out = h.release();
  });
}
int swn_ctx_destroy(swn_ctx* ctx) {
  return guard([&] {
    if (!ctx) return;
    delete ctx;           // the context itself goes with its last model / pipeline
  });
}
int swn_ctx_set_overlap(swn_ctx* ctx, int on) {
  return guard([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c->join_side();
    stream_sync(ctx->c->s);
    ctx->c->side_enabled = on != 0;
  });
}
int swn_ctx_attach_comm(swn_ctx* ctx, swn_allreduce_fn fn, void* comm, int world_size) {
  return guard([&] {
    REQUIRE(ctx, "ctx is NULL");
    ctx->c->join_side();
    ctx->c->attach_comm(reinterpret_cast<Ctx::AllReduceFn>(fn), comm, fn ? world_size : 1);
  });
}
int swn_ctx_set_patchgan_layers(swn_ctx* ctx, int n_layers) {
  return guard([&] {
    REQUIRE(ctx, "ctx is NULL");
    REQUIRE(n_layers >= 0 && n_layers <= 5, "n_layers_D must be in [1, 5], or 0 for the 1x1 PixelDiscriminator");
    ctx->c->patchgan_layers = n_layers;
  });
}
int swn_ctx_set_patchgan_norm(swn_ctx* ctx, int kind) {
  return guard([&] {
    REQUIRE(ctx, "ctx is NULL");
    REQUIRE(kind >= 0 && kind <= 2, "normalization layer is not found (0 instance, 1 batch, 2 none)");
    ctx->c->patchgan_norm = kind;
  });
}
int swn_ctx_sync(swn_ctx* ctx) {
  return guard([&] { REQUIRE(ctx, "ctx is NULL"); stream_sync(ctx->c->s); });
}
int swn_ctx_bytes_allocated(swn_ctx* ctx, size_t* out) {
  return guard([&] { REQUIRE(ctx && out, "NULL argument"); *out = ctx->c->bytes_allocated; });
}

int swn_prof_enable(int on) { return guard([&] { prof_enable(on); }); }
int swn_prof_reset(void) { return guard([&] { prof_reset(); }); }
int swn_prof_report(char* buf, int len) { return prof_report(buf, len); }
int swn_probe_mfma(swn_ctx* ctx, int zeros, int iters, float* out4) {
  return guard([&] {
    REQUIRE(ctx && out4, "swn_probe_mfma: NULL argument");
    REQUIRE(iters >= 1 && iters <= (1 << 20), "swn_probe_mfma: iters out of range");
    probe_mfma(ctx->c->s, zeros, iters, out4);
  });
}
int swn_route_trace(int on) { return guard([&] { route_enable(on); }); }
int swn_route_report(char* buf, int len) { return route_report(buf, len); }
int swn_slot_audit(int on) { return guard([&] { slot_audit(on); }); }
// recorded launch sequences are never audited (the audit reads back): off for the duration of the call
struct AuditSuspend {
  int was = slot_audit_on();
  AuditSuspend() { slot_audit(0); }
  ~AuditSuspend() { slot_audit(was); }
};

int swn_warp_model_create_ex(swn_ctx* ctx, int batch, int height, int width, int is_train, float dropout,
                             int body_channels, int cloth_channels, swn_model** out) {
  return guard([&] {
    REQUIRE(ctx && out, "NULL argument");
    REQUIRE(batch > 0 && height > 0 && width > 0, "bad shape");
    auto h = std::make_unique<swn_model>();
    h->keep = ctx->box;
    h->m.reset(create_warp_model(*ctx->c, batch, height, width, is_train != 0, dropout, body_channels, cloth_channels));
    h->kind = 0; h->is_train = is_train != 0; h->dropout = dropout; h->body_channels = body_channels; h->cloth_channels = cloth_channels;
    h->patchgan_layers = ctx->c->patchgan_layers; h->patchgan_norm = ctx->c->patchgan_norm;
    *out = h.release();
  });
}
int swn_warp_model_create(swn_ctx* ctx, int batch, int height, int width, int is_train, float dropout,
                          swn_model** out) {
  return swn_warp_model_create_ex(ctx, batch, height, width, is_train, dropout, 3, 19, out);
}
int swn_texture_model_create_netG(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                                  int cloth_channels, int netG, swn_model** out) {
  return guard([&] {
    REQUIRE(ctx && out, "NULL argument");
    auto h = std::make_unique<swn_model>();
    h->keep = ctx->box;
    h->m.reset(create_texture_model(*ctx->c, batch, height, width, is_train != 0, num_roi, cloth_channels, nullptr, netG));
    h->kind = 1; h->is_train = is_train != 0; h->num_roi = num_roi; h->cloth_channels = cloth_channels;
    h->patchgan_layers = ctx->c->patchgan_layers; h->netG = netG;
    *out = h.release();
  });
}
int swn_texture_model_create_ex(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                                int cloth_channels, swn_model** out) {
  return swn_texture_model_create_netG(ctx, batch, height, width, is_train, num_roi, cloth_channels, NETG_SWAPNET, out);
}
int swn_texture_model_create(swn_ctx* ctx, int batch, int height, int width, int is_train, int num_roi,
                             swn_model** out) {
  return swn_texture_model_create_ex(ctx, batch, height, width, is_train, num_roi, 19, out);
}
int swn_model_create_shared(swn_model* sharer, int batch, int height, int width, swn_model** out) {
  return guard([&] {
    REQUIRE(sharer && out, "NULL argument");
    REQUIRE(batch > 0 && height > 0 && width > 0, "bad shape");
    std::shared_ptr<Model> root = sharer->sharer ? sharer->sharer : sharer->m;        // always the owner of the arenas
    Ctx& c = *root->ctx;
    auto h = std::make_unique<swn_model>();
    h->keep = sharer->keep;
    h->sharer = root;
    h->kind = sharer->kind; h->is_train = sharer->is_train; h->dropout = sharer->dropout; h->num_roi = sharer->num_roi;
    h->body_channels = sharer->body_channels; h->cloth_channels = sharer->cloth_channels; h->patchgan_layers = sharer->patchgan_layers;
    h->patchgan_norm = sharer->patchgan_norm; h->netG = sharer->netG;
    const int layers_was = c.patchgan_layers, norm_was = c.patchgan_norm;
    c.patchgan_layers = sharer->patchgan_layers; c.patchgan_norm = sharer->patchgan_norm;
    try {
      if (h->kind == 0)
        h->m.reset(create_warp_model(c, batch, height, width, h->is_train != 0, h->dropout, h->body_channels, h->cloth_channels, root.get()));
      else
        h->m.reset(create_texture_model(c, batch, height, width, h->is_train != 0, h->num_roi, h->cloth_channels, root.get(), h->netG));
    } catch (...) { c.patchgan_layers = layers_was; c.patchgan_norm = norm_was; throw; }
    c.patchgan_layers = layers_was; c.patchgan_norm = norm_was;
    h->m->hyper = root->hyper;
    *out = h.release();
  });
}
int swn_model_destroy(swn_model* m) {
  return guard([&] { delete m; });
}

int swn_model_set_hyper(swn_model* m, const swn_hyper* h) {
  return guard([&] {
    REQUIRE(m && h, "NULL argument");
    const Hyper before = m->m->hyper;
    struct Recheck {          // a recorded step (swn_model_step_captured) carries the hyper-parameters it was recorded with
      Model& mm; const Hyper& was;
      ~Recheck() { if (memcmp(&was, &mm.hyper, sizeof(Hyper)) != 0) mm.invalidate_step_graphs(); }
    } recheck{*m->m, before};
    Hyper& y = m->m->hyper;
    y.lr = h->lr; y.d_lr = h->d_lr; y.weight_decay = h->weight_decay; y.d_weight_decay = h->d_weight_decay;
    y.b1 = h->b1; y.b2 = h->b2; y.lambda_gan = h->lambda_gan; y.lambda_ce = h->lambda_ce; y.lambda_l1 = h->lambda_l1;
    y.lambda_content = h->lambda_content; y.lambda_style = h->lambda_style;
    REQUIRE(h->gan_mode >= 0 && h->gan_mode <= 2, "gan mode not implemented");
    y.gan_mode = h->gan_mode; y.warp_mode_ce_only = h->warp_mode_ce;
    y.grad_scale = h->grad_scale > 0.f ? h->grad_scale : 1.f;
    // negative = inherit optimizer_G's value; 0 is a legitimate beta (WGAN-GP style (0, 0.9) betas)
    y.d_b1 = h->d_b1 >= 0.f ? h->d_b1 : h->b1; y.d_b2 = h->d_b2 >= 0.f ? h->d_b2 : h->b2;
    REQUIRE(h->gp_mode >= 0 && h->gp_mode <= 3, "gradient penalty mode not implemented");
    REQUIRE(h->gp_mode == 0 || m->m->supports_gradient_penalty(),
            "gradient penalty modes are not implemented for the texture model (the reference's call fails there too), for the "
            "1x1 PixelDiscriminator, nor -- on the host simulator -- for a discriminator under --norm batch / none (the second-order "
            "pass through BatchNorm and without a norm layer is in the device library only)");
    y.gp_mode = h->gp_mode; y.lambda_gp = h->lambda_gp;
  });
}

static ParamArena& arena_of(swn_model* m, int net) {
  REQUIRE(m, "model is NULL");
  ParamArena* a = m->m->arena_ptr(net);
  REQUIRE(a, "this model has no such network");
  return *a;
}

int swn_model_set_optimizer(swn_model* m, int net, int kind, float final_lr, float base_lr, float gamma) {
  return guard([&] {
    REQUIRE(net == 0 || net == 1, "optimizers exist for the generator (0) and the discriminator (1)");
    ParamArena& a = arena_of(m, net);
    REQUIRE(m->m->is_train, "the model was created without optimizers (is_train = 0)");
    REQUIRE(kind == OPT_ADAMW || kind == OPT_ADABOUND, "optimizer kind not implemented (0 AdamW, 1 AdaBound)");
    if (kind == OPT_ADABOUND) {
      // the simulator's update is AdamW whatever the kind says: refuse here, not at the first step
      if (!is_device_build()) throw Error(1, "swn_model_set_optimizer: AdaBound is not implemented on the host simulator (HIP kernel only)");
      REQUIRE(final_lr >= 0.f && base_lr > 0.f && gamma > 0.f, "AdaBound needs final_lr >= 0, base_lr > 0, gamma > 0");
    }
    // a recorded step (swn_model_step_captured) launches the kernel of the kind it was recorded with
    if (a.opt_kind != kind || (kind == OPT_ADABOUND && (a.final_lr != final_lr || a.base_lr != base_lr || a.gamma != gamma)))
      m->m->invalidate_step_graphs();
    a.opt_kind = kind;
    if (kind == OPT_ADABOUND) { a.final_lr = final_lr; a.base_lr = base_lr; a.gamma = gamma; }
  });
}

int swn_model_param_count(swn_model* m, int net, int* out) {
  return guard([&] { REQUIRE(out, "NULL"); *out = (int)arena_of(m, net).params.size(); });
}
int swn_model_param_info(swn_model* m, int net, int index, char* name, int name_len, int shape[4], int* ndim) {
  return guard([&] {
    ParamArena& a = arena_of(m, net);
    REQUIRE(index >= 0 && index < (int)a.params.size(), "param index out of range");
    const ParamDesc& d = a.params[index];
    if (name && name_len > 0) { std::strncpy(name, d.name.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (d.is_bias) {
      if (shape) { shape[0] = d.n_logical; shape[1] = shape[2] = shape[3] = 1; }
      if (ndim) *ndim = 1;
    } else {
      if (shape) {
        if (d.ws.kind == WK_CONV) { shape[0] = d.ws.Co; shape[1] = d.ws.Ci; }
        else { shape[0] = d.ws.Ci; shape[1] = d.ws.Co; }
        shape[2] = d.ws.KH; shape[3] = d.ws.KW;
      }
      if (ndim) *ndim = 4;
    }
  });
}
static const ParamDesc& find_param(ParamArena& a, const char* name) {
  REQUIRE(name, "name is NULL");
  auto it = a.index.find(name);
  if (it == a.index.end()) throw Error(1, std::string("unknown parameter ") + name);
  return a.params[it->second];
}
int swn_model_param_set(swn_model* m, int net, int which, const char* name, const float* src) {
  return guard([&] {
    ParamArena& a = arena_of(m, net);
    REQUIRE(which >= 0 && which <= 3 && src, "bad argument");
    const ParamDesc& d = find_param(a, name);
    Stream& s = m->m->ctx->s;
    if (d.is_bias) dev_copy(s, a.base(which) + d.off, src, d.n_logical * sizeof(float));
    else pack_weight(s, d.ws, src, a.base(which) + d.off);
    if (which == 0) a.version += 1;
  });
}
int swn_model_param_get(swn_model* m, int net, int which, const char* name, float* dst) {
  return guard([&] {
    ParamArena& a = arena_of(m, net);
    REQUIRE(which >= 0 && which <= 3 && dst, "bad argument");
    const ParamDesc& d = find_param(a, name);
    Stream& s = m->m->ctx->s;
    if (d.is_bias) dev_copy(s, dst, a.base(which) + d.off, d.n_logical * sizeof(float));
    else unpack_weight(s, d.ws, a.base(which) + d.off, dst);
  });
}
// ---- state-dict buffers: the running statistics of the BatchNorm sites of the discriminator (--norm batch) and of the
// texture stage's unet_128 generator -----------------------------------------------------------------------------------------
static std::vector<Model::BNSite>& sites_of(swn_model* m, int net) {
  static std::vector<Model::BNSite> none;
  arena_of(m, net);                      // (validates the model and the network)
  return net == 0 || net == 1 ? m->m->bn_sites(net) : none;
}
static const char* const kBufferNames[3] = {"running_mean", "running_var", "num_batches_tracked"};
static void* find_buffer(swn_model* m, int net, const char* name, size_t* bytes) {
  REQUIRE(name, "name is NULL");
  const std::string full(name);
  for (Model::BNSite& s : sites_of(m, net))
    for (int k = 0; k < 3; ++k)
      if (full == s.name + "." + kBufferNames[k]) {
        *bytes = k == 2 ? sizeof(int64_t) : (size_t)s.C * sizeof(float);
        return k == 0 ? (void*)s.run.mean : k == 1 ? (void*)s.run.var : (void*)s.run.count;
      }
  throw Error(1, std::string("unknown buffer ") + name);
}
int swn_model_buffer_count(swn_model* m, int net, int* out) {
  return guard([&] { REQUIRE(out, "NULL"); *out = 3 * (int)sites_of(m, net).size(); });
}
int swn_model_buffer_info(swn_model* m, int net, int index, char* name, int name_len, int* numel, int* is_int64) {
  return guard([&] {
    auto& sites = sites_of(m, net);
    REQUIRE(index >= 0 && index < 3 * (int)sites.size(), "buffer index out of range");
    const Model::BNSite& s = sites[index / 3];
    const std::string full = s.name + "." + kBufferNames[index % 3];
    if (name && name_len > 0) { std::strncpy(name, full.c_str(), name_len - 1); name[name_len - 1] = 0; }
    if (numel) *numel = index % 3 == 2 ? 1 : s.C;
    if (is_int64) *is_int64 = index % 3 == 2;
  });
}
int swn_model_buffer_set(swn_model* m, int net, const char* name, const void* src) {
  return guard([&] {
    REQUIRE(src, "NULL argument");
    size_t bytes = 0;
    void* dst = find_buffer(m, net, name, &bytes);
    dev_copy(m->m->ctx->s, dst, src, bytes);
  });
}
int swn_model_buffer_get(swn_model* m, int net, const char* name, void* dst) {
  return guard([&] {
    REQUIRE(dst, "NULL argument");
    size_t bytes = 0;
    const void* src = find_buffer(m, net, name, &bytes);
    dev_copy(m->m->ctx->s, dst, src, bytes);
  });
}
int swn_model_set_discriminate_mode(swn_model* m, int training) {
  return guard([&] { REQUIRE(m, "NULL argument"); m->m->discriminate_training = training != 0; });
}
int swn_model_optim_step_get(swn_model* m, int net, int* step) {
  return guard([&] { REQUIRE(step, "NULL"); *step = arena_of(m, net).step; });
}
int swn_model_optim_step_set(swn_model* m, int net, int step) {
  return guard([&] { arena_of(m, net).step = step; });
}

int swn_model_set_input(swn_model* m, int slot, const float* src, int n, int c, int h, int w) {
  return guard([&] { REQUIRE(m && src, "NULL argument"); m->m->set_input(slot, src, n, c, h, w); });
}
int swn_model_set_input_labels(swn_model* m, int slot, const int32_t* lab, int n, int h, int w) {
  return guard([&] { REQUIRE(m && lab, "NULL argument"); m->m->set_input_labels(slot, lab, n, h, w); });
}
int swn_model_set_input_texture_batch(swn_model* m, const uint8_t* img, int b, int hs, int ws, const uint8_t* labels, int hl, int wl,
                                      const float* rois_raw, int r, const float* sample, const float* mean3, const float* std3,
                                      int x_min, int y_min) {
  return guard([&] {
    REQUIRE(m && img && labels && rois_raw && sample && mean3 && std3, "NULL argument");
    m->m->set_input_texture_batch(img, b, hs, ws, labels, hl, wl, rois_raw, r, sample, mean3, std3, x_min, y_min);
  });
}
int swn_model_set_input_texture_sources(swn_model* m, const uint8_t* src, size_t src_bytes, const int64_t* geom_host, int b, int hs, int ws,
                                        const uint8_t* labels, int hl, int wl, const float* rois_raw, int r, const float* sample,
                                        const float* mean3, const float* std3, int x_min, int y_min) {
  return guard([&] {
    REQUIRE(m && src && geom_host && labels && rois_raw && sample && mean3 && std3, "NULL argument");
    m->m->set_input_texture_sources(src, src_bytes, geom_host, b, hs, ws, labels, hl, wl, rois_raw, r, sample, mean3, std3, x_min, y_min);
  });
}
int swn_model_set_input_warp_batch(swn_model* m, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels,
                                   const uint8_t* tgt_labels, int hl, int wl, const double* maps, int nmaps, const float* mean3,
                                   const float* std3, int load_size, int x_min, int y_min) {
  return swn_model_set_input_warp_batch_ex(m, body, b, hb, wb, in_labels, tgt_labels, hl, wl, maps, nmaps, mean3, std3, load_size, x_min, y_min, 0);
}
int swn_model_set_input_warp_batch_ex(swn_model* m, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels,
                                      const uint8_t* tgt_labels, int hl, int wl, const double* maps, int nmaps, const float* mean3,
                                      const float* std3, int load_size, int x_min, int y_min, int flags) {
  return guard([&] {
    REQUIRE(m && body && in_labels && mean3 && std3, "NULL argument");
    REQUIRE((flags & ~1) == 0, "set_input_warp_batch: unknown flag bits");
    m->m->set_input_warp_batch(body, b, hb, wb, in_labels, tgt_labels, hl, wl, maps, nmaps, mean3, std3, load_size, x_min, y_min, flags);
  });
}
int swn_model_get_output(swn_model* m, int slot, float* dst) {
  return guard([&] { REQUIRE(m && dst, "NULL argument"); m->m->get_output(slot, dst); });
}
int swn_model_get_tap_grad(swn_model* m, int net, const char* name, float* dst, int shape[4]) {
  return guard([&] {
    REQUIRE(m && name, "NULL argument");
    Net* n = m->m->net_for_taps(net);
    REQUIRE(n, "no such network");
    auto it = n->taps.find(name);
    if (it == n->taps.end()) throw Error(1, std::string("unknown tap ") + name);
    REQUIRE(it->second.has_grad, "tap carries no gradient");
    const TView& v = it->second.g;
    if (shape) { shape[0] = v.N; shape[1] = v.C; shape[2] = v.H; shape[3] = v.W; }
    if (dst) nhwc_to_nchw(m->m->ctx->s, v, dst, v.C);
  });
}
int swn_model_get_tap(swn_model* m, int net, const char* name, float* dst, int shape[4]) {
  return guard([&] {
    REQUIRE(m && name, "NULL argument");
    Net* n = m->m->net_for_taps(net);
    REQUIRE(n, "no such network");
    auto it = n->taps.find(name);
    if (it == n->taps.end()) throw Error(1, std::string("unknown tap ") + name);
    const TView& v = it->second.v;
    if (shape) { shape[0] = v.N; shape[1] = v.C; shape[2] = v.H; shape[3] = v.W; }
    if (dst) nhwc_to_nchw(m->m->ctx->s, v, dst, v.C);
  });
}
int swn_model_dropout_sites(swn_model* m, int net, int* count) {
  return guard([&] {
    REQUIRE(m && count, "NULL argument");
    Net* n = m->m->net_for_taps(net);
    REQUIRE(n, "no such network");
    *count = (int)n->drop_sites.size();
  });
}
int swn_model_dropout_mask(swn_model* m, int net, int site, uint64_t seed, float* dst, int shape[4], float* p) {
  return guard([&] {
    REQUIRE(m, "NULL argument");
    Net* n = m->m->net_for_taps(net);
    REQUIRE(n, "no such network");
    REQUIRE(site >= 0 && site < (int)n->drop_sites.size(), "dropout site out of range");
    const Net::DropSite& d = n->drop_sites[site];
    if (shape) { shape[0] = d.N; shape[1] = d.C; shape[2] = d.H; shape[3] = d.W; }
    if (p) *p = d.p;
    if (dst) dropout_mask(m->m->ctx->s, d.N, d.H, d.W, d.C, d.p, Net::drop_seed(seed, d.salt), dst);
  });
}
int swn_model_act_sites(swn_model* m, int net, int* count) {
  return guard([&] {
    REQUIRE(m && count, "NULL argument");
    Net* n = m->m->net_for_patterns(net);
    REQUIRE(n, "no such network");
    *count = (int)n->act_sites.size();
  });
}
int swn_model_act_pattern(swn_model* m, int net, int site, uint8_t* dst, int shape[4], int* kind) {
  return guard([&] {
    REQUIRE(m, "NULL argument");
    Net* n = m->m->net_for_patterns(net);
    REQUIRE(n, "no such network");
    REQUIRE(site >= 0 && site < (int)n->act_sites.size(), "activation site out of range");
    const Net::ActSite& a = n->act_sites[site];
    if (shape) { shape[0] = a.y.N; shape[1] = a.y.C; shape[2] = a.y.H; shape[3] = a.y.W; }
    if (kind) *kind = a.kind;
    if (dst) {
      if (a.kind == 2) pool_pattern(m->m->ctx->s, a.x, a.y, dst);
      else act_pattern(m->m->ctx->s, a.y, dst);
    }
  });
}
int swn_model_set_style_context(swn_model* m, const float* all_out, const float* all_tgt, int n_total, int n0) {
  return guard([&] { REQUIRE(m && all_out && all_tgt, "NULL argument"); m->m->set_style_context(all_out, all_tgt, n_total, n0); });
}
int swn_model_set_gp_random(swn_model* m, const float* alpha, const float* beta) {
  return guard([&] { REQUIRE(m, "NULL argument"); m->m->set_gp_random(alpha, beta); });
}
int swn_model_discriminate(swn_model* m, const float* x, float* pred) {
  return guard([&] { REQUIRE(m && x && pred, "NULL argument"); m->m->discriminate(x, pred); });
}
int swn_model_perceptual(swn_model* m, const float* output, const float* target, int use_style, float* out2,
                         float content_w, float style_w, float* d_output) {
  return guard([&] {
    REQUIRE(m && output && target && out2, "NULL argument");
    m->m->perceptual(output, target, use_style, out2, content_w, style_w, d_output);
  });
}
int swn_pipeline_create(swn_model* warp, swn_model* texture, swn_pipeline** out) {
  return guard([&] {
    REQUIRE(warp && texture && out, "NULL argument");
    // the two-stage hand-off feeds the texture generator's cloth input, which the plain U-Net does not have
    REQUIRE(texture->kind != 1 || texture->netG == NETG_SWAPNET,
            "swn_pipeline_create: a --netG unet_128 texture model is not implemented (the hand-off feeds a cloth input this generator does not have)");
    auto h = std::make_unique<swn_pipeline>();
    h->keep = warp->keep;
    h->p = std::make_unique<Pipeline>(*warp->m, *texture->m);
    *out = h.release();
  });
}
int swn_pipeline_destroy(swn_pipeline* p) {
  return guard([&] { delete p; });
}
int swn_pipeline_run(swn_pipeline* p, int use_graph, int* graph_replayed) {
  return guard([&] {
    REQUIRE(p, "NULL argument");
    const bool had = p->p->graph_captured();
    std::unique_ptr<AuditSuspend> unaudited(use_graph ? new AuditSuspend : nullptr);
    p->p->run(use_graph != 0);
    if (graph_replayed) *graph_replayed = (use_graph && had) ? 1 : 0;
  });
}
int swn_pipeline_labels(swn_pipeline* p, int32_t** dev_labels) {
  return guard([&] { REQUIRE(p && dev_labels, "NULL argument"); *dev_labels = p->p->labels(); });
}
int swn_pipeline_enable_images(swn_pipeline* p, const float* body_mean3, const float* body_std3, const float* tex_mean3,
                               const float* tex_std3, const uint8_t* colours, int width, int reference_quirk) {
  return guard([&] {
    REQUIRE(p && body_mean3 && body_std3 && tex_mean3 && tex_std3 && colours, "NULL argument");
    p->p->enable_images(body_mean3, body_std3, tex_mean3, tex_std3, colours, width, reference_quirk != 0);
  });
}
int swn_pipeline_images(swn_pipeline* p, uint8_t** dev, int* k) {
  return guard([&] {
    REQUIRE(p && dev && k, "NULL argument");
    REQUIRE(p->p->images(), "swn_pipeline_images: the pipeline was not armed (swn_pipeline_enable_images)");
    *dev = p->p->images(); *k = Pipeline::IMAGE_SHEETS;
  });
}
// (util/util.py:54-69 save_image: the PNG encoding of the sheet, on the device)
int swn_pipeline_enable_png(swn_pipeline* p, int rows_per_chunk) {
  return guard([&] { REQUIRE(p, "NULL argument"); p->p->enable_png(rows_per_chunk); });
}
int swn_pipeline_png(swn_pipeline* p, uint8_t** streams, uint32_t** sizes, size_t* stride, int* k) {
  return guard([&] {
    REQUIRE(p && streams && sizes && stride && k, "NULL argument");
    REQUIRE(p->p->png_streams(), "swn_pipeline_png: the pipeline was not armed (swn_pipeline_enable_png)");
    *streams = p->p->png_streams(); *sizes = p->p->png_sizes(); *stride = p->p->png_stride(); *k = Pipeline::IMAGE_SHEETS;
  });
}
int swn_model_forward(swn_model* m, int training, uint64_t seed) {
  return guard([&] { REQUIRE(m, "NULL"); m->m->forward(training != 0, seed); });
}
int swn_model_backward_D(swn_model* m, float lf, float lr) {
  return guard([&] { REQUIRE(m && m->m->is_train, "model was not created for training"); m->m->backward_D(lf, lr); });
}
int swn_model_backward_G(swn_model* m, float lr) {
  return guard([&] { REQUIRE(m && m->m->is_train, "model was not created for training"); m->m->backward_G(lr); });
}
int swn_model_backward_G_parts(swn_model* m, int* nparts) {
  return guard([&] { REQUIRE(m && nparts, "NULL argument"); *nparts = m->m->backward_G_parts(); });
}
int swn_model_backward_G_part(swn_model* m, float lr, int part, size_t* off, size_t* count) {
  return guard([&] {
    REQUIRE(m && m->m->is_train && part >= 0 && part < m->m->backward_G_parts(), "bad argument");
    m->m->backward_G_part(lr, part, off, count);
  });
}
int swn_model_optimizer_step(swn_model* m, int net) {
  return guard([&] {
    REQUIRE(m && m->m->is_train, "model was not created for training");
    REQUIRE(net == 0 || net == 1, "net must be 0 (G) or 1 (D)");
    m->m->optimizer_step(net);
  });
}
int swn_model_optimizer_step_range(swn_model* m, int net, size_t off, size_t count, int first) {
  return guard([&] {
    REQUIRE(m && m->m->is_train, "model was not created for training");
    REQUIRE(net == 0 || net == 1, "net must be 0 (G) or 1 (D)");
    m->m->optimizer_step_range(net, off, count, first);
  });
}
int swn_model_step(swn_model* m, const float labels[3], int training, uint64_t seed) {
  return guard([&] {
    REQUIRE(m && labels && m->m->is_train, "model was not created for training");
    m->m->step(labels, training != 0, seed);
  });
}
int swn_model_step_dp(swn_model* m, const float labels[3], int training, uint64_t seed, int after_forward) {
  return guard([&] {
    REQUIRE(m && labels && m->m->is_train, "model was not created for training");
    m->m->step_dp(labels, training != 0, seed, after_forward != 0);
  });
}
int swn_model_step_captured(swn_model* m, const float labels[3], int training, uint64_t seed) {
  return guard([&] {
    REQUIRE(m && labels && m->m->is_train, "model was not created for training");
    AuditSuspend unaudited;
    m->m->step_captured(labels, training != 0, seed);
  });
}
int swn_model_get_losses(swn_model* m, float* host_out, int n) {
  return guard([&] {
    REQUIRE(m && host_out && n > 0 && n <= L_COUNT, "bad argument");
    dev_download(m->m->ctx->s, host_out, m->m->losses, n * sizeof(float));
  });
}
int swn_model_grad_arena(swn_model* m, int net, float** p, size_t* count) {
  return guard([&] { ParamArena& a = arena_of(m, net); REQUIRE(p && count, "NULL"); *p = a.g; *count = a.n; });
}
int swn_model_weight_arena(swn_model* m, int net, float** p, size_t* count) {
  return guard([&] { ParamArena& a = arena_of(m, net); REQUIRE(p && count, "NULL"); *p = a.w; *count = a.n; a.version += 1; });
}

int swn_model_arena(swn_model* m, int net, int which, float** p, size_t* count) {
  return guard([&] {
    ParamArena& a = arena_of(m, net);
    REQUIRE(p && count && which >= 0 && which <= 3, "bad argument");
    *p = a.base(which); *count = a.n;
    if (which == 0) a.version += 1;
  });
}

// ---- operator level -----------------------------------------------------------------------
int swn_op_roi_align(swn_ctx* ctx, const float* tex, int b, int c, int h, int w, const float* rois, int r, int ph,
                     int pw, float* out) {
  return guard([&] {
    REQUIRE(ctx && tex && rois && out, "NULL argument");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var t = net.alloc_var(b, h, w, round_up(c, 4), false);
    Var o = net.alloc_var(b, ph, pw, round_up(r * c, 4), false);
    nchw_to_nhwc(tmp.s, tex, b, c, h, w, t.v);
    roi_align_fwd(tmp.s, t.v, c, rois, r, o.v);
    nhwc_to_nchw(tmp.s, o.v, out, r * c);
    stream_sync(tmp.s);
  });
}
int swn_op_roi_align_indices(swn_ctx* ctx, const float* rois, int k, int h, int w, int ph, int pw, int32_t* idx,
                             uint8_t* valid) {
  return guard([&] {
    REQUIRE(ctx && rois && idx && valid, "NULL argument");
    roi_align_indices(ctx->c->s, rois, k, h, w, ph, pw, idx, valid);
    stream_sync(ctx->c->s);
  });
}
int swn_op_decode_labels(swn_ctx* ctx, const float* x, int b, int c, int h, int w, uint8_t* rgb) {
  return guard([&] {
    REQUIRE(ctx && x && rgb, "NULL argument");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var t = net.alloc_var(b, h, w, round_up(c, 4), false);
    nchw_to_nhwc(tmp.s, x, b, c, h, w, t.v);
    decode_labels(tmp.s, t.v, c, rgb);
    stream_sync(tmp.s);
  });
}
int swn_op_image_u8(swn_ctx* ctx, const float* x, int b, int c, int h, int w, const int32_t* labels, int source, const float* rows,
                    int scale_each, int range, const float* rois, int r, const uint8_t* colours, int width, uint8_t* out) {
  return guard([&] {
    REQUIRE(ctx && out, "NULL argument");
    REQUIRE(b > 0 && h > 0 && w > 0, "image_u8: empty sizes");
    REQUIRE(source == SRC_LABELS ? (labels && !x) : (x && !labels), "image_u8: x for the float and argmax sources, labels (and a NULL x) for SRC_LABELS");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    ImageU8Args a;
    a.source = source; a.rows = rows; a.scale_each = scale_each; a.range = range; a.rois = rois; a.R = r; a.colours = colours; a.width = width;
    a.out = out;
    if (source == SRC_LABELS) {
      a.labels = labels; a.B = b; a.H = h; a.W = w;
    } else {
      REQUIRE(c >= 1 && c <= 256, "image_u8: 1 to 256 channels");
      Var t = net.alloc_var(b, h, w, round_up(c, 4), false);        // pad channels zero: a 3-in-4 view, as the models hold theirs
      nchw_to_nhwc(tmp.s, x, b, c, h, w, t.v);
      a.x = t.v; a.C = c;
      if (scale_each) a.minmax = static_cast<float*>(tmp.alloc((size_t)b * image_u8_chunks(h, w) * 2 * sizeof(float)));
    }
    image_u8(tmp.s, a);
    stream_sync(tmp.s);
  });
}
// (util/util.py:54-69 save_image: Image.fromarray(a).save(path) -- its filtering and deflate)
int swn_op_png_encode(swn_ctx* ctx, const uint8_t* img, int n, int h, int w, int rows_per_chunk, uint8_t* streams, size_t stream_stride,
                      uint32_t* sizes) {
  return guard([&] {
    REQUIRE(ctx && img && streams && sizes, "NULL argument");
    REQUIRE(n > 0, "png_encode: empty batch");
    const PngGeom g = png_geometry(h, w, rows_per_chunk);
    REQUIRE(stream_stride >= g.bound, "png_encode: stream_stride is below swn_png_stream_bound");
    Ctx tmp(ctx->c->s);
    PngEncodeArgs a;
    a.img = img; a.n = n; a.h = h; a.w = w; a.rows_per_chunk = rows_per_chunk; a.streams = streams; a.stream_stride = stream_stride; a.sizes = sizes;
    a.scratch = tmp.alloc(png_scratch_bytes(n, g));
    png_encode(tmp.s, a);
    stream_sync(tmp.s);
  });
}
int swn_png_stream_bound(int h, int w, int rows_per_chunk, size_t* out) {
  return guard([&] { REQUIRE(out, "NULL argument"); *out = png_geometry(h, w, rows_per_chunk).bound; });
}
int swn_op_argmax_labels(swn_ctx* ctx, const float* x, int b, int c, int h, int w, int32_t* labels) {
  return guard([&] {
    REQUIRE(ctx && x && labels, "NULL argument");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var t = net.alloc_var(b, h, w, round_up(c, 4), false);
    nchw_to_nhwc(tmp.s, x, b, c, h, w, t.v);
    argmax_labels(tmp.s, t.v, c, labels);
    stream_sync(tmp.s);
  });
}
int swn_op_labels_to_onehot(swn_ctx* ctx, const int32_t* labels, int b, int c, int h, int w, float* out) {
  return guard([&] {
    REQUIRE(ctx && labels && out, "NULL argument");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var t = net.alloc_var(b, h, w, round_up(c, 4), false);
    labels_to_onehot(tmp.s, labels, t.v, c);
    nhwc_to_nchw(tmp.s, t.v, out, c);
    stream_sync(tmp.s);
  });
}

int swn_op_conv(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w,
                float* wgt, int co, const float* bias, int act, float* y) {
  return guard([&] {
    REQUIRE(ctx && x && wgt && y, "NULL argument");
    REQUIRE(kind >= 0 && kind <= 5 && what >= 0 && what <= 2, "bad kind/what");
    REQUIRE(what == 0 || act == ACT_NONE, "backward entry points take the gradient of the pre-activation output");
    // (set before the net is built: with the checkers forced no pre-cut-only operands are planned)
    struct Restore { ~Restore() { conv_force_naive(0); } } restore;
    conv_force_naive(naive);
    Ctx tmp(ctx->c->s);
    ParamArena A;
    Net net(tmp, A);
    const int Cip = round_up(ci, 4), Cop = round_up(co, 4);
    int Ho, Wo;
    if (transposed) { Ho = 2 * h; Wo = 2 * w; }
    else if (kind == CK_K4S2) { Ho = h / 2; Wo = w / 2; }
    else if (kind == CK_K4S1) { Ho = h - 1; Wo = w - 1; }
    else if (kind == CK_TAIL_UP) { Ho = 2 * h; Wo = 2 * w; }
    else { Ho = h; Wo = w; }
    Var xv = net.alloc_var(n, h, w, Cip, true);
    Var yv = net.alloc_var(n, Ho, Wo, Cop, true);
    if (transposed) { REQUIRE(Cip == ci, "transposed conv needs Ci % 4 == 0"); net.convT("l", xv, yv, co, bias != nullptr); }
    else net.conv("l", xv, yv, (ConvKind)kind, ci, co, bias != nullptr, act);
    A.allocate(tmp);
    net.finalize({});
    Stream& s = tmp.s;
    const ParamDesc& wd = A.params[A.index.at("l.weight")];
    if (what != 2) nchw_to_nhwc(s, x, n, ci, h, w, xv.v);
    if (what != 1) pack_weight(s, wd.ws, wgt, A.w + wd.off);
    if (bias) dev_copy(s, A.w + A.params[A.index.at("l.bias")].off, bias, co * sizeof(float));
    if (what == 0) {
      net.forward();
      nhwc_to_nchw(s, yv.v, y, co);
    } else {
      nchw_to_nhwc(s, y, n, co, Ho, Wo, yv.g);
      if (what == 1) {
        net.refresh_dgrad();        // a layer that is not the net's first also forms its input gradient: from operands that exist
        net.backward(true, false);
        unpack_weight(s, wd.ws, A.g + wd.off, wgt);
      } else {
        A.version += 1;
        net.refresh_dgrad();
        net.backward(false, true);
        nhwc_to_nchw(s, xv.g, x, ci);
      }
    }
    stream_sync(s);
  });
}

int swn_op_conv_produced(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w,
                         float* wgt, int co, const float* bias, int act, float* y, int pre, int post, float* x_out, float* x_slot,
                         float* y_slot, float* z_slot, float* dy_out, float* dy_slot, int* kscale_out) {
  return guard([&] {
    REQUIRE(ctx && x && wgt && y, "NULL argument");
    REQUIRE(kind >= 0 && kind <= 5 && what >= 0 && what <= 2, "bad kind/what");
    REQUIRE(what == 0 || act == ACT_NONE, "backward entry points take the gradient of the pre-activation output");
    REQUIRE(pre >= 0 && pre <= 4 && post >= 0 && post <= 1, "bad pre/post stage");
    REQUIRE(pre != 3 || (h % 2 == 0 && w % 2 == 0), "pre = upsample needs an even conv input");
    REQUIRE(what != 0 || (!dy_out && !dy_slot), "dy_out / dy_slot belong to the backward calls");
    struct Restore { ~Restore() { conv_force_naive(0); } } restore;
    conv_force_naive(naive);
    Ctx tmp(ctx->c->s);
    ParamArena A;
    Net net(tmp, A);
    const int Cip = round_up(ci, 4), Cop = round_up(co, 4);
    int Ho, Wo;
    if (transposed) { Ho = 2 * h; Wo = 2 * w; }
    else if (kind == CK_K4S2) { Ho = h / 2; Wo = w / 2; }
    else if (kind == CK_K4S1) { Ho = h - 1; Wo = w - 1; }
    else if (kind == CK_TAIL_UP) { Ho = 2 * h; Wo = 2 * w; }
    else { Ho = h; Wo = w; }
    // x0 -> [pre] -> x -> [conv] -> y -> [post] -> z: the conv's operands x and y.g are written by kernels of ours, on the tape
    const int h0 = pre == 3 ? h / 2 : (pre == 4 ? 2 * h : h), w0 = pre == 3 ? w / 2 : (pre == 4 ? 2 * w : w);
    Var x0 = net.alloc_var(n, h0, w0, Cip, false);
    Var xv = net.alloc_var(n, h, w, Cip, true);
    Var yv = net.alloc_var(n, Ho, Wo, Cop, true);
    Var zv = net.alloc_var(n, Ho, Wo, Cop, true);
    if (pre == 0) net.norm_act(x0, xv, false, ACT_NONE, 0.f);
    else if (pre == 1) net.norm_act(x0, xv, true, ACT_LRELU, 0.f);
    else if (pre == 2) net.act(x0, xv, ACT_RELU);
    else if (pre == 3) net.upsample(x0, xv, 2);
    else net.maxpool(x0, xv);
    if (transposed) { REQUIRE(Cip == ci, "transposed conv needs Ci % 4 == 0"); net.convT("l", xv, yv, co, bias != nullptr); }
    else net.conv("l", xv, yv, (ConvKind)kind, ci, co, bias != nullptr, act);
    net.norm_act(yv, zv, post == 1, post == 1 ? ACT_LRELU : ACT_NONE, 0.f);
    A.allocate(tmp);
    net.finalize({});
    Stream& s = tmp.s;
    const ParamDesc& wd = A.params[A.index.at("l.weight")];
    auto slot_of = [&](const float* base, const char* whose) -> const float* {
      auto it = net.buf_slots.find(base);
      if (it == net.buf_slots.end() || !it->second.complete || !net.amax) throw Error(1, std::string("swn_op_conv_produced: ") + whose + " has no complete amax slot on this route");
      return net.amax + it->second.off;
    };
    auto copy_slot = [&](float* dst, const float* base, const char* whose) {
      if (dst) dev_copy(s, dst, slot_of(base, whose), AMAX_SLOT * sizeof(float));
    };
    // (the backward calls run the forward pass too: it zeroes the slots and lets the producer of x fold)
    if (what != 2) nchw_to_nhwc(s, x, n, ci, h0, w0, x0.v);
    else dev_memset(s, x0.v.p, 0, x0.v.pixels() * x0.v.cs * sizeof(float));
    pack_weight(s, wd.ws, wgt, A.w + wd.off);       // (what 1: the forward pass in front of the backward one runs on them)
    if (bias) dev_copy(s, A.w + A.params[A.index.at("l.bias")].off, bias, co * sizeof(float));
    net.forward();
    if (x_out) nhwc_to_nchw(s, xv.v, x_out, ci);
    copy_slot(x_slot, xv.vbase, "x");
    copy_slot(y_slot, yv.vbase, "y");
    copy_slot(z_slot, zv.vbase, "z");
    if (what == 0) {
      nhwc_to_nchw(s, zv.v, y, co);
    } else {
      nchw_to_nhwc(s, y, n, co, Ho, Wo, zv.g);
      if (what == 1) {
        net.refresh_dgrad();
        net.backward(true, false);
        unpack_weight(s, wd.ws, A.g + wd.off, wgt);
      } else {
        A.version += 1;
        net.refresh_dgrad();
        net.backward(false, true);
        nhwc_to_nchw(s, xv.g, x, ci);
      }
      if (dy_out) nhwc_to_nchw(s, yv.g, dy_out, co);
      copy_slot(dy_slot, yv.gbase, "y.g");
    }
    if (kscale_out && net.kscale_n) dev_copy(s, kscale_out, net.kscale, std::min<size_t>(net.kscale_n, 8) * sizeof(int));
    stream_sync(s);
  });
}

int swn_op_instance_norm_act(swn_ctx* ctx, const float* x, int n, int c, int h, int w, int act, float* y) {
  return guard([&] {
    REQUIRE(ctx && x && y && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true);
    net.norm_act(xv, yv, true, act, 0.f);
    net.finalize({});
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nhwc_to_nchw(tmp.s, yv.v, y, c);
    stream_sync(tmp.s);
  });
}
int swn_op_instance_norm_act_bwd(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int act,
                                 float* dx) {
  return guard([&] {
    REQUIRE(ctx && x && dy && dx && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true);
    net.norm_act(xv, yv, true, act, 0.f);
    net.finalize({});
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nchw_to_nhwc(tmp.s, dy, n, c, h, w, yv.g);
    net.backward(false, true);
    nhwc_to_nchw(tmp.s, xv.g, dx, c);
    stream_sync(tmp.s);
  });
}
// BatchNorm2d + activation as one call (tests, tools/bn_shapes.py): the layer of Net::batch_norm_act on NCHW tensors
static void bn_op_build(Ctx& tmp, ParamArena& A, Net& net, Var& xv, Var& yv, int n, int c, int h, int w, int groups, int act,
                        const Net::BNBuffers& run, const float* weight, const float* bias) {
  xv = net.alloc_var(n, h, w, c, true); yv = net.alloc_var(n, h, w, c, true);
  net.batch_norm_act("bn", xv, yv, act, groups, run);
  A.allocate(tmp);
  net.finalize({});
  dev_copy(tmp.s, A.w + A.params[A.index.at("bn.weight")].off, weight, c * sizeof(float));
  dev_copy(tmp.s, A.w + A.params[A.index.at("bn.bias")].off, bias, c * sizeof(float));
}
int swn_op_batch_norm_act(swn_ctx* ctx, const float* x, int n, int c, int h, int w, int groups, int act, int training,
                          const float* weight, const float* bias, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float* y, float* save_stats) {
  return guard([&] {
    REQUIRE(ctx && x && y && weight && bias && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    REQUIRE(training || (running_mean && running_var), "eval mode needs the running buffers");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv, yv;
    Net::BNBuffers run{running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked)};
    bn_op_build(tmp, A, net, xv, yv, n, c, h, w, groups, act, run, weight, bias);
    net.bn_training = training != 0;
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nhwc_to_nchw(tmp.s, yv.v, y, c);
    if (save_stats && training) dev_copy(tmp.s, save_stats, net.last_stats, (size_t)groups * c * 2 * sizeof(float));
    stream_sync(tmp.s);
  });
}
int swn_op_batch_norm_act_bwd(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int groups, int act,
                              const float* weight, const float* bias, float* dx, float* dweight, float* dbias) {
  return guard([&] {
    REQUIRE(ctx && x && dy && dx && weight && bias && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    REQUIRE((dweight != nullptr) == (dbias != nullptr), "dweight and dbias go together");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv, yv;
    bn_op_build(tmp, A, net, xv, yv, n, c, h, w, groups, act, Net::BNBuffers(), weight, bias);
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nchw_to_nhwc(tmp.s, dy, n, c, h, w, yv.g);
    net.backward(dweight != nullptr, true);
    nhwc_to_nchw(tmp.s, xv.g, dx, c);
    if (dweight) {
      dev_copy(tmp.s, dweight, A.g + A.params[A.index.at("bn.weight")].off, c * sizeof(float));
      dev_copy(tmp.s, dbias, A.g + A.params[A.index.at("bn.bias")].off, c * sizeof(float));
    }
    stream_sync(tmp.s);
  });
}
// BatchNorm2d -> [act] -> Dropout(p), training mode, as one call: the fused site of Net::batch_norm_act(..., drop_p)
int swn_op_batch_norm_act_dropout(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int act, float p,
                                  uint64_t seed, const float* weight, const float* bias, float* y, float* mask, float* dx,
                                  float* dweight, float* dbias) {
  return guard([&] {
    REQUIRE(ctx && x && y && weight && bias && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    REQUIRE(p >= 0.f && p < 1.f, "dropout probability must be in [0, 1)");
    REQUIRE((dy != nullptr) == (dx != nullptr), "dy and dx go together");
    REQUIRE((dweight != nullptr) == (dbias != nullptr) && (!dweight || dy), "dweight and dbias go together and need dy / dx");
    REQUIRE(!mask || p > 0.f, "mask requested with p == 0");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true);
    net.batch_norm_act("bn", xv, yv, act, 1, Net::BNBuffers(), p);
    A.allocate(tmp);
    net.finalize({});
    dev_copy(tmp.s, A.w + A.params[A.index.at("bn.weight")].off, weight, c * sizeof(float));
    dev_copy(tmp.s, A.w + A.params[A.index.at("bn.bias")].off, bias, c * sizeof(float));
    net.training = true; net.bn_training = true; net.seed = seed;
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nhwc_to_nchw(tmp.s, yv.v, y, c);
    if (mask) {
      const Net::DropSite& d = net.drop_sites.at(0);
      dropout_mask(tmp.s, d.N, d.H, d.W, d.C, d.p, Net::drop_seed(seed, d.salt), mask);
    }
    if (dy) {
      nchw_to_nhwc(tmp.s, dy, n, c, h, w, yv.g);
      net.backward(dweight != nullptr, true);
      nhwc_to_nchw(tmp.s, xv.g, dx, c);
      if (dweight) {
        dev_copy(tmp.s, dweight, A.g + A.params[A.index.at("bn.weight")].off, c * sizeof(float));
        dev_copy(tmp.s, dbias, A.g + A.params[A.index.at("bn.bias")].off, c * sizeof(float));
      }
    }
    stream_sync(tmp.s);
  });
}
int swn_op_norm_act_time(swn_ctx* ctx, int kind, int what, const float* x, const float* dy, int n, int c, int h, int w, int groups,
                         int act, int warmup, int iters, float* ms_out) {
  return guard([&] {
    REQUIRE(ctx && x && ms_out && c % 4 == 0 && (what == 0 || dy), "bad argument (C must be a multiple of 4; the backward pass needs dy)");
    REQUIRE((kind == 0 || kind == 1) && (what == 0 || what == 1) && warmup >= 0 && iters >= 1 && iters <= 1000, "bad kind / what / iters");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true);
    if (kind == 0) {
      net.norm_act(xv, yv, true, act, 0.f);
    } else {
      // gamma = 1, beta = 0; fresh running buffers, updated by every forward pass like a training step's
      float* run = static_cast<float*>(tmp.alloc((size_t)2 * c * sizeof(float) + 16));
      net.batch_norm_act("bn", xv, yv, act, groups, Net::BNBuffers{run, run + c, reinterpret_cast<long long*>(run + 2 * c)});
      A.allocate(tmp);
      std::vector<float> ones(c, 1.f);
      dev_upload(tmp.s, A.w + A.params[A.index.at("bn.weight")].off, ones.data(), c * sizeof(float));
    }
    net.finalize({});
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    if (what == 1) nchw_to_nhwc(tmp.s, dy, n, c, h, w, yv.g);
    time_launches(tmp.s, warmup, iters, [&] { if (what == 0) net.forward(); else net.backward(true, true); }, ms_out);
  });
}
int swn_op_affine_gather(swn_ctx* ctx, const float* src, float* dst, int b, int c, int h, int w, const double* maps,
                         int nmaps) {
  return guard([&] {
    REQUIRE(ctx && src && dst && maps, "NULL argument");
    REQUIRE(src != dst, "affine_gather is out of place");
    affine_gather(ctx->c->s, src, dst, b, c, h, w, maps, nmaps);
  });
}
int swn_op_chain_resample(swn_ctx* ctx, const float* src, float* dst, int b, int c, int h, int w, const double* maps,
                          int nmaps) {
  return guard([&] {
    REQUIRE(ctx && src && dst && maps, "NULL argument");
    REQUIRE(src != dst, "chain_resample is out of place");
    chain_resample(ctx->c->s, src, dst, b, c, h, w, maps, nmaps);
  });
}
int swn_op_texture_batch(swn_ctx* ctx, const uint8_t* img, int b, int hs, int ws, const uint8_t* labels, int hl, int wl,
                         const float* rois_raw, int r, const float* sample, const float* mean3, const float* std3, int x_min,
                         int y_min, int h, int w, int cloth_channels, float* in_nchw, float* tgt_nchw, float* cloths_nchw,
                         float* rois_out) {
  return guard([&] {
    REQUIRE(ctx && img && labels && rois_raw && sample && mean3 && std3 && in_nchw && tgt_nchw && cloths_nchw && rois_out, "NULL argument");
    REQUIRE(b > 0 && h > 0 && w > 0, "texture_batch: empty sizes");
    REQUIRE(cloth_channels >= 1 && cloth_channels <= 64, "texture_batch: cloth channels in [1,64]");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    // one buffer [input texel | target texel | one-hot], so that every destination is a channel slice like the model's
    const int cp = round_up(cloth_channels, 4);
    Var t = net.alloc_var(b, h, w, 8 + cp, false);
    TextureBatchArgs a;
    a.img = img; a.Hs = hs; a.Ws = ws; a.labels = labels; a.Hl = hl; a.Wl = wl; a.rois_raw = rois_raw; a.R = r; a.sample = sample;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.std[c] = std3[c]; }
    a.x_min = x_min; a.y_min = y_min; a.C = cloth_channels;
    a.in_tex = t.v.slice(0, 4); a.tgt_tex = t.v.slice(4, 4); a.cloth[0] = t.v.slice(8, cp); a.ncloth = 1;
    a.rois_out = rois_out;
    texture_batch(tmp.s, a);
    nhwc_to_nchw(tmp.s, a.in_tex, in_nchw, 3);
    nhwc_to_nchw(tmp.s, a.tgt_tex, tgt_nchw, 3);
    nhwc_to_nchw(tmp.s, a.cloth[0], cloths_nchw, cloth_channels);
    stream_sync(tmp.s);
  });
}
int swn_op_resize_u8(swn_ctx* ctx, const uint8_t* src, size_t src_bytes, const int64_t* geom_host, int b, int hs, int ws, uint8_t* dst) {
  return guard([&] {
    REQUIRE(ctx && src && geom_host && dst, "NULL argument");
    ResizeU8Args a;
    a.src = src; a.src_bytes = src_bytes; a.geom = geom_host; a.B = b; a.Hs = hs; a.Ws = ws; a.dst = dst;
    resize_u8(ctx->c->s, a);                 // enqueued only: no allocation, no synchronisation
  });
}
int swn_op_warp_batch(swn_ctx* ctx, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels, const uint8_t* tgt_labels, int hl,
                      int wl, const double* maps, int nmaps, const float* mean3, const float* std3, int load_size, int x_min, int y_min,
                      int h, int w, int cloth_channels, float* bodys_nchw, float* input_cloths_nchw, float* target_cloths_nchw) {
  return swn_op_warp_batch_ex(ctx, body, b, hb, wb, in_labels, tgt_labels, hl, wl, maps, nmaps, mean3, std3, load_size, x_min, y_min, h, w,
                              cloth_channels, bodys_nchw, input_cloths_nchw, target_cloths_nchw, 0);
}
int swn_op_warp_batch_ex(swn_ctx* ctx, const uint8_t* body, int b, int hb, int wb, const uint8_t* in_labels, const uint8_t* tgt_labels, int hl,
                         int wl, const double* maps, int nmaps, const float* mean3, const float* std3, int load_size, int x_min, int y_min,
                         int h, int w, int cloth_channels, float* bodys_nchw, float* input_cloths_nchw, float* target_cloths_nchw,
                         int flags) {
  return guard([&] {
    REQUIRE(ctx && body && in_labels && mean3 && std3 && bodys_nchw && input_cloths_nchw, "NULL argument");
    REQUIRE((flags & ~1) == 0, "warp_batch: unknown flag bits");
    REQUIRE(!target_cloths_nchw || tgt_labels, "warp_batch: target cloths asked for without target label maps");
    REQUIRE(b > 0 && h > 0 && w > 0, "warp_batch: empty sizes");
    REQUIRE(cloth_channels >= 2 && cloth_channels <= 64, "warp_batch: cloth channels in [2,64]");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    // one buffer [body texel | input cloth | target cloth], so that every destination is a channel slice like the model's
    const int cp = round_up(cloth_channels, 4);
    Var t = net.alloc_var(b, h, w, 4 + 2 * cp, false);
    WarpBatchArgs a;
    a.body = body; a.Hb = hb; a.Wb = wb; a.in_labels = in_labels; a.Hl = hl; a.Wl = wl; a.maps = maps; a.nmaps = nmaps;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.std[c] = std3[c]; }
    a.Ls = load_size; a.x_min = x_min; a.y_min = y_min; a.C = cloth_channels; a.bicubic = (flags & 1) != 0;
    a.body_out[0] = t.v.slice(0, 4); a.nbody = 1; a.in_cloth = t.v.slice(4, cp);
    if (target_cloths_nchw) { a.tgt_labels = tgt_labels; a.tgt_cloth = t.v.slice(4 + cp, cp); }
    warp_batch(tmp.s, a);
    nhwc_to_nchw(tmp.s, a.body_out[0], bodys_nchw, 3);
    nhwc_to_nchw(tmp.s, a.in_cloth, input_cloths_nchw, cloth_channels);
    if (target_cloths_nchw) nhwc_to_nchw(tmp.s, a.tgt_cloth, target_cloths_nchw, cloth_channels);
    stream_sync(tmp.s);
  });
}
int swn_op_gan_loss(swn_ctx* ctx, int gan_mode, const float* pred, int n, int c, int h, int w, float label,
                    int target_is_real, float grad_scale, float* loss_out, float* dpred) {
  return guard([&] {
    REQUIRE(ctx && pred && loss_out, "NULL argument");
    REQUIRE(gan_mode >= 0 && gan_mode <= 2, "gan mode not implemented");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    // the prediction map (N,C,H,W) is reduced over all of its elements: view it as N*C single-channel images
    Var pv = net.alloc_var(n * c, h, w, 4, true);
    nchw_to_nhwc(tmp.s, pred, n * c, 1, h, w, pv.v);
    float* lo = static_cast<float*>(tmp.alloc(sizeof(float)));
    const TView* dp = dpred ? &pv.g : nullptr;
    if (gan_mode == 0) bce_logits_loss(tmp.s, pv.v, label, grad_scale, lo, dp);
    else if (gan_mode == 1) lsgan_loss(tmp.s, pv.v, label, grad_scale, lo, dp);
    else wgan_loss(tmp.s, pv.v, target_is_real ? -1.f : 1.f, grad_scale, lo, dp);
    dev_copy(tmp.s, loss_out, lo, sizeof(float));
    if (dpred) nhwc_to_nchw(tmp.s, pv.g, dpred, 1);
    stream_sync(tmp.s);
  });
}
// 0x7f7f7f7f = 3.39e38f in every pad channel: a kernel that sums a pad shows it at once, one that writes a pad changes the bits, and
// 0 + sentinel keeps them (an accumulating kernel that adds zero into a pad leaves it as it was)
static const int kPadSentinelByte = 0x7f;
int swn_op_loss(swn_ctx* ctx, int kind, const float* a, const float* b, int n, int c, int h, int w, int pad_c, float scale,
                int accumulate, int n0, int nloc, float* loss_out, float* da, float* pad_out) {
  return guard([&] {
    REQUIRE(ctx && a && b && loss_out, "NULL argument");
    REQUIRE(kind >= 0 && kind <= 3, "bad loss kind");
    REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && pad_c >= 0 && (c + pad_c) % 4 == 0, "bad shape (c + pad_c must be a multiple of 4)");
    REQUIRE(!pad_out || (da && pad_c > 0), "pad_out needs a gradient and pad channels");
    if (kind != 3 || nloc < 0) { n0 = 0; nloc = n; }
    REQUIRE(n0 >= 0 && nloc >= 1 && n0 + nloc <= n, "bad n0 / nloc");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Stream& s = tmp.s;
    const int cp = c + pad_c;
    Var av = net.alloc_var(n, h, w, cp, false), bv = net.alloc_var(n, h, w, cp, false);
    Var gv = net.alloc_var(nloc, h, w, cp, false);           // the gradient view: nloc samples (gram_style_loss), else the batch
    for (const TView* t : {&av.v, &bv.v, &gv.v}) dev_memset(s, t->p, kPadSentinelByte, t->pixels() * t->cs * sizeof(float));
    nchw_to_nhwc(s, a, n, c, h, w, av.v);
    nchw_to_nhwc(s, b, n, c, h, w, bv.v);
    if (da && accumulate) nchw_to_nhwc(s, da, nloc, c, h, w, gv.v);
    // the logical channels as a slice of the wider buffer (cs > C); cross entropy takes the rounded-up slice, as the nets pass it
    const int cv = kind == 0 ? round_up(c, 4) : c;
    const TView va = av.v.slice(0, cv), vb = bv.v.slice(0, cv), vg = gv.v.slice(0, cv);
    const TView* dp = da ? &vg : nullptr;
    float* lo = static_cast<float*>(tmp.alloc(sizeof(float)));
    if (kind == 0) ce_argmax_loss(s, va, vb, c, scale, lo, dp, accumulate);
    else if (kind == 1) l1_loss(s, va, vb, c, scale, lo, dp, accumulate);
    else if (kind == 2) normed_mse_loss(s, va, vb, scale, lo, dp, accumulate);
    else gram_style_loss(s, va, vb, c, scale, lo, dp, accumulate, n0, nloc);
    dev_copy(s, loss_out, lo, sizeof(float));
    if (da) nhwc_to_nchw(s, gv.v, da, c);
    if (pad_out) nhwc_to_nchw(s, gv.v.slice(c, pad_c), pad_out, pad_c);
    stream_sync(s);
  });
}
int swn_op_bias_grad(swn_ctx* ctx, const float* dy, int n, int c, int h, int w, int pad_c, float* db) {
  return guard([&] {
    REQUIRE(ctx && dy && db, "NULL argument");
    REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h > 0 && w > 0 && pad_c >= 0 && pad_c % 4 == 0, "bad shape (c and pad_c must be multiples of 4)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Stream& s = tmp.s;
    Var yv = net.alloc_var(n, h, w, c + pad_c, false);
    dev_memset(s, yv.v.p, kPadSentinelByte, yv.v.pixels() * yv.v.cs * sizeof(float));
    nchw_to_nhwc(s, dy, n, c, h, w, yv.v);
    float* out = static_cast<float*>(tmp.alloc((size_t)c * sizeof(float)));
    bias_grad(s, yv.v.slice(0, c), out);
    dev_copy(s, db, out, (size_t)c * sizeof(float));
    stream_sync(s);
  });
}
// (modules/losses/__init__.py:128-259 SSIM and :14-27 L1_Charbonnier_loss; enqueued only: no allocation, no synchronisation)
int swn_op_ssim(swn_ctx* ctx, const float* img1, const float* img2, int b, int c, int h, int w, int window, float max_val,
                float* loss_map, float* loss_sum, const float* gmap, float gscalar, float* d1, float* d2) {
  return guard([&] {
    REQUIRE(ctx && img1 && img2 && loss_sum, "NULL argument");
    SsimArgs a;
    a.img1 = img1; a.img2 = img2; a.B = b; a.C = c; a.H = h; a.W = w; a.window = window; a.max_val = max_val;
    a.loss_map = loss_map; a.loss_sum = loss_sum; a.gmap = gmap; a.gscalar = gscalar; a.d1 = d1; a.d2 = d2;
    ssim_loss(ctx->c->s, a);
  });
}
int swn_op_charbonnier(swn_ctx* ctx, const float* x, const float* y, size_t n, float eps, float gscalar, float* loss_sum, float* dx,
                       float* dy) {
  return guard([&] {
    REQUIRE(ctx && x && y && loss_sum, "NULL argument");
    CharbonnierArgs a;
    a.x = x; a.y = y; a.n = n; a.eps = eps; a.gscalar = gscalar; a.loss_sum = loss_sum; a.dx = dx; a.dy = dy;
    charbonnier_loss(ctx->c->s, a);
  });
}
// ---- the kernels between the convolutions on channel-slice views (swapnet_hip.h: swn_op_norm_act / _elementwise / _resample) ----
// one operand: an (N,H,W,lead + c + pad) buffer, every byte the sentinel, the logical channels loaded into slice(lead, c)
struct OpBuf { TView whole, v; };
static OpBuf op_buf(Net& net, Stream& s, int n, int h, int w, int c, const int* lp, const float* nchw) {
  REQUIRE(lp[0] >= 0 && lp[1] >= 0 && lp[0] % 4 == 0 && lp[1] % 4 == 0, "lead_c and pad_c must be non-negative multiples of 4");
  OpBuf b;
  b.whole = net.alloc_var(n, h, w, lp[0] + c + lp[1], false).v;
  dev_memset(s, b.whole.p, kPadSentinelByte, b.whole.pixels() * b.whole.cs * sizeof(float));
  b.v = b.whole.slice(lp[0], c);
  if (nchw) nchw_to_nhwc(s, nchw, n, c, h, w, b.v);
  return b;
}
static void op_buf_out(Stream& s, const OpBuf& b, float* nchw, float* whole_nchw) {
  if (nchw) nhwc_to_nchw(s, b.v, nchw, b.v.C);
  if (whole_nchw) nhwc_to_nchw(s, b.whole, whole_nchw, b.whole.C);
}
static float* op_slot(Ctx& tmp, bool want) {
  if (!want) return nullptr;
  float* p = static_cast<float*>(tmp.alloc(AMAX_SLOT * sizeof(float)));
  dev_memset(tmp.s, p, 0, AMAX_SLOT * sizeof(float));
  return p;
}
int swn_op_norm_act(swn_ctx* ctx, const float* x, const float* dy, const float* residual, int n, int c, int h, int w, int norm,
                    int act, float drop_p, uint64_t seed, int seed_on_device, uint64_t salt, const double* partial_in,
                    int partial_chunks, const int* lead_pad, int want_colsum, float* y, float* stats, float* y_slot, float* dx,
                    float* dx_slot, double* colsum, int* colsum_emitted, float* db, float* y_buf, float* dx_buf) {
  return guard([&] {
    REQUIRE(ctx && x && lead_pad && (y || dy), "NULL argument");
    REQUIRE(y || !norm || stats, "the backward pass alone (y == NULL) takes the statistics from `stats`");
    REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h > 0 && w > 0, "bad shape (C must be a multiple of 4)");
    REQUIRE(act >= 0 && act <= 3 && drop_p >= 0.f && drop_p < 1.f, "bad activation / dropout probability must be in [0, 1)");
    REQUIRE((dy != nullptr) == (dx != nullptr), "dy and dx go together");
    REQUIRE(want_colsum >= 0 && want_colsum <= 2 && (!want_colsum || dy), "bad want_colsum (column sums belong to the backward pass)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Stream& s = tmp.s;
    OpBuf xb = op_buf(net, s, n, h, w, c, lead_pad, x), yb = op_buf(net, s, n, h, w, c, lead_pad + 2, nullptr), rb;
    if (residual) rb = op_buf(net, s, n, h, w, c, lead_pad + 8, residual);
    float* st = static_cast<float*>(tmp.alloc((size_t)n * c * 2 * sizeof(float)));
    uint64_t* seed_dev = nullptr;
    if (seed_on_device) {
      seed_dev = static_cast<uint64_t*>(tmp.alloc(sizeof(uint64_t)));
      dev_upload(s, seed_dev, &seed, sizeof(uint64_t));
    }
    NormActArgs a;
    a.x = xb.v; a.y = yb.v; a.stats = st; a.norm = norm; a.act = act; a.drop_p = drop_p;
    a.seed = seed_on_device ? 0 : seed; a.seed_base = seed_dev; a.salt = salt;
    a.residual = residual ? &rb.v : nullptr;
    a.amax_out = op_slot(tmp, y && y_slot);
    a.partial_in = partial_in; a.partial_chunks = partial_chunks;
    if (y) {
      norm_act_fwd(s, a);
      op_buf_out(s, yb, y, y_buf);
      if (stats && norm) dev_copy(s, stats, st, (size_t)n * c * 2 * sizeof(float));
      if (y_slot) dev_copy(s, y_slot, a.amax_out, AMAX_SLOT * sizeof(float));
    } else if (norm) {
      dev_copy(s, st, stats, (size_t)n * c * 2 * sizeof(float));
    }
    if (colsum_emitted) *colsum_emitted = 0;
    if (dy) {
      OpBuf gb = op_buf(net, s, n, h, w, c, lead_pad + 4, dy), db_ = op_buf(net, s, n, h, w, c, lead_pad + 6, nullptr);
      const bool ask = want_colsum == 2 || (want_colsum == 1 && norm && norm_act_bwd_emits_colsum(h * w, c));
      NormActBwdArgs b;
      b.dy = gb.v; b.x = xb.v; b.stats = st; b.dx = db_.v; b.norm = norm; b.act = act; b.drop_p = drop_p;
      b.seed = a.seed; b.seed_base = seed_dev; b.salt = salt;
      b.colsum = ask ? static_cast<double*>(tmp.alloc((size_t)n * c * sizeof(double))) : nullptr;
      b.amax_out = op_slot(tmp, dx_slot != nullptr);
      norm_act_bwd(s, b);
      op_buf_out(s, db_, dx, dx_buf);
      if (dx_slot) dev_copy(s, dx_slot, b.amax_out, AMAX_SLOT * sizeof(float));
      if (ask) {
        if (colsum_emitted) *colsum_emitted = 1;
        if (colsum) dev_copy(s, colsum, b.colsum, (size_t)n * c * sizeof(double));
        if (db) {
          float* o = static_cast<float*>(tmp.alloc((size_t)c * sizeof(float)));
          bias_grad_from_colsums(s, b.colsum, n, c, o);
          dev_copy(s, db, o, (size_t)c * sizeof(float));
        }
      }
    }
    stream_sync(s);
  });
}
int swn_op_elementwise(swn_ctx* ctx, int op, const float* a, const float* b, int n, int c, int h, int w, int act, int accumulate,
                       float alpha, float shift, const int* lead_pad, float* out, float* slot, float* out_buf) {
  return guard([&] {
    REQUIRE(ctx && a && out && lead_pad && (op != 1 || b), "NULL argument");
    REQUIRE(op >= 0 && op <= 2 && act >= 0 && act <= 3, "bad op / activation");
    REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h > 0 && w > 0, "bad shape (C must be a multiple of 4)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Stream& s = tmp.s;
    OpBuf ab = op_buf(net, s, n, h, w, c, lead_pad, a), bb;
    if (op == 1) bb = op_buf(net, s, n, h, w, c, lead_pad + 2, b);
    OpBuf ob = op_buf(net, s, n, h, w, c, lead_pad + 4, (op != 0 && accumulate) ? out : nullptr);
    float* sl = op_slot(tmp, slot != nullptr);
    if (op == 0) act_fwd(s, ab.v, ob.v, act, sl);
    else if (op == 1) act_bwd(s, ab.v, bb.v, ob.v, act, accumulate, sl);
    else axpy(s, ab.v, ob.v, alpha, accumulate, shift, sl);
    op_buf_out(s, ob, out, out_buf);
    if (slot) dev_copy(s, slot, sl, AMAX_SLOT * sizeof(float));
    stream_sync(s);
  });
}
int swn_op_resample(swn_ctx* ctx, int op, const float* a, const float* b, int n, int c, int h, int w, int factor, int accumulate,
                    const int* lead_pad, float* out, float* slot, uint8_t* pattern, float* out_buf) {
  return guard([&] {
    REQUIRE(ctx && a && lead_pad && (out || op == 5) && (op != 3 || b), "NULL argument");
    REQUIRE(op >= 0 && op <= 5, "bad op");
    REQUIRE(n > 0 && c > 0 && c % 4 == 0 && h > 0 && w > 0, "bad shape (C must be a multiple of 4)");
    if (op >= 2) factor = 2;
    REQUIRE(factor >= 1 && (op == 0 || op >= 4 || (h % factor == 0 && w % factor == 0)), "bad factor (h and w must be multiples of it)");
    REQUIRE(op != 4 || (h > 2 && w > 2), "reflect_fold: the padded gradient is at least 3 x 3");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Stream& s = tmp.s;
    // geometry of the output and of the pooled map
    const int ho = op == 0 ? h * factor : (op == 1 || op == 2) ? h / factor : op == 4 ? h - 2 : h;
    const int wo = op == 0 ? w * factor : (op == 1 || op == 2) ? w / factor : op == 4 ? w - 2 : w;
    OpBuf ab = op_buf(net, s, n, h, w, c, lead_pad, a);
    float* sl = op_slot(tmp, slot != nullptr);
    uint8_t* pat = nullptr;
    const size_t pat_bytes = (size_t)n * c * (op == 5 ? (size_t)h * w : (size_t)(h / 2) * (w / 2));
    if (pattern) {
      REQUIRE(op == 2 || op == 3 || op == 5, "this op has no pattern");
      pat = static_cast<uint8_t*>(tmp.alloc(pat_bytes));
    }
    if (op == 5) {
      REQUIRE(pattern, "act_pattern: pattern is NULL");
      act_pattern(s, ab.v, pat);
    } else {
      OpBuf ob = op_buf(net, s, n, ho, wo, c, lead_pad + 4, accumulate && (op == 1 || op == 3 || op == 4) ? out : nullptr);
      if (op == 0) upsample_nearest_fwd(s, ab.v, ob.v, factor, sl);
      else if (op == 1) upsample_nearest_bwd(s, ab.v, ob.v, factor, accumulate);
      else if (op == 2) {
        maxpool2_fwd(s, ab.v, ob.v, sl);
        if (pat) pool_pattern(s, ab.v, ob.v, pat);
      } else if (op == 3) {
        OpBuf gb = op_buf(net, s, n, h / 2, w / 2, c, lead_pad + 2, b), yb = op_buf(net, s, n, h / 2, w / 2, c, lead_pad + 2, nullptr);
        maxpool2_fwd(s, ab.v, yb.v, nullptr);
        maxpool2_bwd(s, gb.v, ab.v, yb.v, ob.v, accumulate);
        if (pat) pool_pattern(s, ab.v, yb.v, pat);
      } else reflect_fold(s, ab.v, ob.v, accumulate);
      op_buf_out(s, ob, out, out_buf);
    }
    if (pat) dev_copy(s, pattern, pat, pat_bytes);
    if (slot) dev_copy(s, slot, sl, AMAX_SLOT * sizeof(float));
    stream_sync(s);
  });
}
// ---- one convolution on views, as the networks call it (swapnet_hip.h: swn_op_conv_views) ----
namespace {
// one operand of swn_op_conv_views: value and gradient parents of (n_lead + n + n_pad) x H x W x (lead + cv + pad), every byte the
// sentinel, and the view parent.batch(n_lead, n).slice(lead, cv) the conv gets
struct ConvOperand { Var parent, view; };
ConvOperand conv_operand(Net& net, Stream& s, int n, int h, int w, int cv, const int* g) {
  REQUIRE(g[0] >= 0 && g[1] >= 0 && g[0] % 4 == 0 && g[1] % 4 == 0, "lead_c and pad_c must be non-negative multiples of 4");
  REQUIRE(g[2] >= 0 && g[3] >= 0, "n_lead and n_pad must be non-negative");
  ConvOperand o;
  o.parent = net.alloc_var(g[2] + n + g[3], h, w, g[0] + cv + g[1], true);
  for (const TView* t : {&o.parent.v, &o.parent.g}) dev_memset(s, t->p, kPadSentinelByte, t->pixels() * t->cs * sizeof(float));
  o.view = o.parent.batch(g[2], n).slice(g[0], cv);
  return o;
}
// channel j of image i of a view, as a 1 x H x W x 1 view
TView plane_of(const TView& v, int i, int j) {
  TView r = v;
  r.p = v.p + (size_t)i * v.H * v.W * v.cs + j;
  r.N = 1; r.C = 1;
  return r;
}
// Loads a view: its non-logical channels (map entry -1, or at and above c_log without a map) with zeros, its logical channels with
// nchw (n, c_log, h, w), or leaves them as they are (nchw == NULL).  zeros = n * H * W device zeros.
void view_load(Stream& s, const TView& v, const float* nchw, int c_log, const std::vector<int32_t>& map, const float* zeros) {
  const size_t hw = (size_t)v.H * v.W;
  for (int j = 0; j < v.C; ++j) {
    const int src = map.empty() ? (j < c_log ? j : -1) : map[j];
    if (src < 0) { nchw_to_nhwc(s, zeros, v.N, 1, v.H, v.W, v.slice(j, 1)); continue; }
    if (!nchw || map.empty()) continue;
    for (int i = 0; i < v.N; ++i) nchw_to_nhwc(s, nchw + ((size_t)i * c_log + src) * hw, 1, 1, v.H, v.W, plane_of(v, i, j));
  }
  if (nchw && map.empty()) nchw_to_nhwc(s, nchw, v.N, c_log, v.H, v.W, v);
}
void view_store(Stream& s, const TView& v, float* nchw, int c_log, const std::vector<int32_t>& map) {
  if (map.empty()) { nhwc_to_nchw(s, v, nchw, c_log); return; }
  const size_t hw = (size_t)v.H * v.W;
  for (int j = 0; j < v.C; ++j)
    if (map[j] >= 0)
      for (int i = 0; i < v.N; ++i) nhwc_to_nchw(s, plane_of(v, i, j), nchw + ((size_t)i * c_log + map[j]) * hw, 1);
}
}  // namespace
int swn_op_conv_views(swn_ctx* ctx, int kind, int transposed, int what, int naive, float* x, int n, int ci, int h, int w, float* wgt,
                      int co, const float* bias, int act, float* y, const int* views, const int32_t* cimap, int cimap_len,
                      int x_is_input, int dgrad_C, int operand_slots, const float* dx_old, const int* pre_range, float* y_fwd,
                      float* y_slot, float* dw_rows, float* x_buf, float* xg_buf, float* y_buf, float* yg_buf) {
  return guard([&] {
    REQUIRE(ctx && x && wgt && y && views, "NULL argument");
    REQUIRE(kind >= 0 && kind <= 5 && what >= 0 && what <= 2, "bad kind/what");
    REQUIRE(n > 0 && ci > 0 && co > 0 && h > 0 && w > 0, "bad shape");
    REQUIRE(act >= ACT_NONE && act <= ACT_TANH, "bad activation");
    REQUIRE(what == 0 || act != ACT_TANH, "no network takes a gradient through a fused tanh");
    REQUIRE(!transposed || (act == ACT_NONE && !cimap && !x_is_input && dgrad_C == 0), "a transposed conv has no fused activation, channel map or first-layer option");
    REQUIRE(!dx_old || what == 2, "dx_old belongs to the input-gradient call");
    REQUIRE(!dw_rows || what == 1, "dw_rows belongs to the weight-gradient call");
    REQUIRE(!y_fwd || (what != 0 && act != ACT_NONE), "y_fwd: the forward output of a backward call with a fused activation");
    std::vector<int32_t> map;
    if (cimap) {
      REQUIRE(cimap_len > 0 && cimap_len % 4 == 0, "cimap: one entry per view channel of x (a multiple of 4)");
      map.assign(cimap, cimap + cimap_len);
      std::vector<char> seen(ci, 0);
      int logical = 0;
      for (int32_t m : map) {
        REQUIRE(m >= -1 && m < ci, "cimap: entries are -1 or a logical channel");
        if (m >= 0) { REQUIRE(!seen[m], "cimap: a logical channel appears twice"); seen[m] = 1; ++logical; }
      }
      REQUIRE(logical == ci, "cimap: ci must be the number of non-negative entries");
    }
    struct Restore { ~Restore() { conv_force_naive(0); } } restore;
    conv_force_naive(naive);
    Ctx tmp(ctx->c->s);
    ParamArena A;
    Net net(tmp, A);
    Stream& s = tmp.s;
    const int Cip = cimap ? cimap_len : round_up(ci, 4), Cop = round_up(co, 4);
    int Ho, Wo;
    if (transposed) { Ho = 2 * h; Wo = 2 * w; }
    else if (kind == CK_K4S2) { Ho = h / 2; Wo = w / 2; }
    else if (kind == CK_K4S1) { Ho = h - 1; Wo = w - 1; }
    else if (kind == CK_TAIL_UP) { Ho = 2 * h; Wo = 2 * w; }
    else { Ho = h; Wo = w; }
    REQUIRE(Ho > 0 && Wo > 0, "the map is too small for this conv");
    ConvOperand xo = conv_operand(net, s, n, h, w, Cip, views), yo = conv_operand(net, s, n, Ho, Wo, Cop, views + 4);
    const Var &xv = xo.view, &yv = yo.view;
    if (transposed) { REQUIRE(Cip == ci, "transposed conv needs Ci % 4 == 0"); net.convT("l", xv, yv, co, bias != nullptr); }
    else net.conv("l", xv, yv, (ConvKind)kind, ci, co, bias != nullptr, act, cimap ? &map : nullptr, x_is_input != 0, dgrad_C);
    A.allocate(tmp);
    // the accumulate flag reaches the kernels through the planner alone, as in a model: x.g holds a gradient already (dx_old), and
    // optionally a further channel range of x's parent does
    std::vector<Var> pre;
    if (dx_old) pre.push_back(xv);
    if (pre_range) {
      REQUIRE(pre_range[0] >= 0 && pre_range[1] > 0 && pre_range[0] + pre_range[1] <= xo.parent.g.C, "pre_range: {c0, c} within x's parent buffer");
      pre.push_back(xo.parent.slice(pre_range[0], pre_range[1]));
    }
    net.finalize(pre);
    // operand_slots: x and dY get the external amax slots a model gives the buffers it fills from outside the tape, and the launches
    // take the slot-scaled / pair-form routes of a training step; without, every launch takes the amax of its operand itself
    float* op_slots = nullptr;
    if (operand_slots) {
      op_slots = static_cast<float*>(tmp.alloc(2 * AMAX_SLOT * sizeof(float)));
      dev_memset(s, op_slots, 0, 2 * AMAX_SLOT * sizeof(float));
      net.set_external_slot(xv.vbase, op_slots);
      net.set_external_slot(yv.gbase, op_slots + AMAX_SLOT);
    }
    const ParamDesc& wd = A.params[A.index.at("l.weight")];
    const std::vector<int32_t> no_map;
    const size_t zn = (size_t)n * std::max(h * w, Ho * Wo);
    float* zeros = static_cast<float*>(tmp.alloc(zn * sizeof(float)));
    dev_memset(s, zeros, 0, zn * sizeof(float));
    const bool fwd_first = what != 0 && act != ACT_NONE;
    view_load(s, xv.v, (what != 2 || fwd_first) ? x : nullptr, ci, map, zeros);
    view_load(s, xv.g, dx_old, ci, map, zeros);
    view_load(s, yv.v, nullptr, co, no_map, zeros);
    view_load(s, yv.g, what != 0 ? y : nullptr, co, no_map, zeros);
    if (op_slots && (what != 2 || fwd_first)) tensor_amax(s, xv.v, op_slots);
    if (op_slots && what != 0) tensor_amax(s, yv.g, op_slots + AMAX_SLOT);
    pack_weight(s, wd.ws, wgt, A.w + wd.off);       // (what 1: the forward pass in front of the backward one runs on them)
    if (bias) dev_copy(s, A.w + A.params[A.index.at("l.bias")].off, bias, co * sizeof(float));
    auto copy_slot = [&] {
      if (!y_slot) return;
      auto it = net.buf_slots.find(yv.vbase);
      if (it == net.buf_slots.end() || !it->second.complete || !net.amax) throw Error(1, "swn_op_conv_views: y has no complete amax slot on this route");
      dev_copy(s, y_slot, net.amax + it->second.off, AMAX_SLOT * sizeof(float));
    };
    if (what == 0) {
      net.forward();
      nhwc_to_nchw(s, yv.v, y, co);
      copy_slot();
    } else {
      REQUIRE(!y_slot || fwd_first, "y_slot: the backward calls run the forward pass only in front of a fused activation");
      if (fwd_first) {
        net.forward();
        if (y_fwd) nhwc_to_nchw(s, yv.v, y_fwd, co);
        copy_slot();
      }
      if (what == 1) {
        net.refresh_dgrad();
        net.backward(true, false);
        unpack_weight(s, wd.ws, A.g + wd.off, wgt);
        if (dw_rows) {            // every packed row, the non-logical ones included: (co, Cip, KH, KW) / transposed (Cip, co, 4, 4)
          WShape all = wd.ws;
          all.Ci = all.Cip; all.cimap = nullptr;
          unpack_weight(s, all, A.g + wd.off, dw_rows);
        }
      } else {
        A.version += 1;
        net.refresh_dgrad();
        net.backward(false, true);
        view_store(s, xv.g, x, ci, map);
      }
    }
    if (x_buf) nhwc_to_nchw(s, xo.parent.v, x_buf, xo.parent.v.C);
    if (xg_buf) nhwc_to_nchw(s, xo.parent.g, xg_buf, xo.parent.g.C);
    if (y_buf) nhwc_to_nchw(s, yo.parent.v, y_buf, yo.parent.v.C);
    if (yg_buf) nhwc_to_nchw(s, yo.parent.g, yg_buf, yo.parent.g.C);
    stream_sync(s);
  });
}
int swn_op_norm_act_bwd2(swn_ctx* ctx, const float* x, const float* gy, const float* u, int n, int c, int h, int w, int act,
                         float* uy, float* ax) {
  return guard([&] {
    REQUIRE(ctx && x && gy && u && uy && ax && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true), uv = net.alloc_var(n, h, w, c, true);
    net.norm_act(xv, yv, true, act, 0.f);
    net.finalize({});
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    nchw_to_nhwc(tmp.s, gy, n, c, h, w, yv.g);
    nchw_to_nhwc(tmp.s, u, n, c, h, w, uv.v);
    net.forward();                                  // InstanceNorm statistics of x
    // the statistics live with the op: fetch them through a second-order call on the same buffers
    NormActBwd2Args b2;
    b2.u = uv.v; b2.gy = yv.g; b2.x = xv.v; b2.stats = net.last_stats; b2.uy = uv.g; b2.ax = xv.g; b2.act = act;
    norm_act_bwd2(tmp.s, b2);
    nhwc_to_nchw(tmp.s, uv.g, uy, c);
    nhwc_to_nchw(tmp.s, xv.g, ax, c);
    stream_sync(tmp.s);
  });
}
// the BatchNorm counterpart: training-mode forward (one group, no running buffers) for stats and fold, then ops.h batch_norm_bwd2
int swn_op_batch_norm_act_bwd2(swn_ctx* ctx, const float* x, const float* gy, const float* u, const float* gamma, const float* beta,
                               int n, int c, int h, int w, int act, float* uy, float* ax, float* dgamma) {
  return guard([&] {
    REQUIRE(ctx && x && gy && u && gamma && beta && uy && ax && dgamma && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    REQUIRE(n > 0 && c > 0 && h > 0 && w > 0, "bad shape");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true), uv = net.alloc_var(n, h, w, c, true);
    float* par = static_cast<float*>(tmp.alloc((size_t)7 * c * sizeof(float)));      // gamma, beta, stats [C][2], fold [2][C], d gamma
    float *gd = par, *bd = par + c, *stats = par + 2 * c, *fold = par + 4 * c, *dg = par + 6 * c;
    dev_copy(tmp.s, gd, gamma, c * sizeof(float));
    dev_copy(tmp.s, bd, beta, c * sizeof(float));
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    nchw_to_nhwc(tmp.s, gy, n, c, h, w, yv.g);
    nchw_to_nhwc(tmp.s, u, n, c, h, w, uv.v);
    BatchNormArgs f;
    f.x = xv.v; f.y = yv.v; f.gamma = gd; f.beta = bd; f.stats = stats; f.fold = fold; f.act = act;
    batch_norm_fwd(tmp.s, f);
    BatchNormBwd2Args b2;
    b2.u = uv.v; b2.gy = yv.g; b2.x = xv.v; b2.stats = stats; b2.fold = fold; b2.gamma = gd;
    b2.uy = uv.g; b2.ax = xv.g; b2.dgamma = dg; b2.act = act;
    batch_norm_bwd2(tmp.s, b2);
    nhwc_to_nchw(tmp.s, uv.g, uy, c);
    nhwc_to_nchw(tmp.s, xv.g, ax, c);
    dev_copy(tmp.s, dgamma, dg, c * sizeof(float));
    stream_sync(tmp.s);
  });
}
int swn_op_norm_act_dropout(swn_ctx* ctx, const float* x, const float* dy, int n, int c, int h, int w, int norm, int act,
                            float p, uint64_t seed, float* y, float* mask, float* dx) {
  return guard([&] {
    REQUIRE(ctx && x && y && c % 4 == 0, "bad argument (C must be a multiple of 4)");
    REQUIRE(p >= 0.f && p < 1.f, "dropout probability must be in [0, 1)");
    Ctx tmp(ctx->c->s);
    ParamArena A; Net net(tmp, A);
    Var xv = net.alloc_var(n, h, w, c, true), yv = net.alloc_var(n, h, w, c, true);
    net.norm_act(xv, yv, norm != 0, act, p);
    net.finalize({});
    net.training = true; net.seed = seed;
    nchw_to_nhwc(tmp.s, x, n, c, h, w, xv.v);
    net.forward();
    nhwc_to_nchw(tmp.s, yv.v, y, c);
    if (mask) {
      if (p > 0.f) {
        const Net::DropSite& d = net.drop_sites.at(0);
        dropout_mask(tmp.s, d.N, d.H, d.W, d.C, d.p, Net::drop_seed(seed, d.salt), mask);
      } else {
        REQUIRE(false, "mask requested with p == 0");
      }
    }
    if (dy && dx) {
      nchw_to_nhwc(tmp.s, dy, n, c, h, w, yv.g);
      net.backward(false, true);
      nhwc_to_nchw(tmp.s, xv.g, dx, c);
    }
    stream_sync(tmp.s);
  });
}
int swn_op_adamw(swn_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                 float eps, float wd, int step) {
  return guard([&] {
    REQUIRE(ctx && p && g && m && v, "NULL argument");
    AdamWArgs a{p, g, m, v, n, lr, b1, b2, eps, wd, step};
    adamw_step(ctx->c->s, a);
    stream_sync(ctx->c->s);
  });
}
int swn_op_adabound(swn_ctx* ctx, float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2,
                    float eps, float wd, float final_lr, float base_lr, float gamma, int step) {
  return guard([&] {
    REQUIRE(ctx && p && g && m && v, "NULL argument");
    REQUIRE(step >= 1 && base_lr > 0.f && gamma > 0.f, "AdaBound needs step >= 1, base_lr > 0, gamma > 0");
    if (!is_device_build()) throw Error(1, "swn_op_adabound: AdaBound is not implemented on the host simulator (HIP kernel only)");
    AdamWArgs a{p, g, m, v, n, lr, b1, b2, eps, wd, step};
    a.kind = OPT_ADABOUND; a.final_lr = final_lr; a.base_lr = base_lr; a.gamma = gamma;
    adamw_step(ctx->c->s, a);
    stream_sync(ctx->c->s);
  });
}

}  // extern "C"
