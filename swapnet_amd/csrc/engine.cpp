// swapnet_amd -- engine core: arenas, op tape, accumulate planner.
#include "engine.h"
#include "png_chunk.h"
#include <memory>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace swn {

// ---- routing trace (ops.h route_*) ------------------------------------------------------
namespace {
int g_route = 0;
std::string g_route_label = "-";
char g_route_phase = '-';
std::vector<std::string> g_route_lines;
std::map<std::string, int> g_route_seen;
}  // namespace
void route_enable(int on) {
  g_route = on;
  if (on) { g_route_lines.clear(); g_route_seen.clear(); g_route_label = "-"; g_route_phase = '-'; }
}
bool route_on() { return g_route != 0; }
void route_label(const char* label, char phase) { g_route_label = label ? label : "-"; g_route_phase = phase; }
void route_note(const char* kernel) {
  if (!g_route) return;
  std::string line = g_route_label + " " + std::string(1, g_route_phase) + " " + kernel;
  if (g_route_seen.emplace(line, 1).second) g_route_lines.push_back(line);
}
// ---- slot audit (ops.h slot_audit) --------------------------------------------------------
namespace { int g_slot_audit = 0; }
void slot_audit(int on) { g_slot_audit = on; }
bool slot_audit_on() { return g_slot_audit != 0; }

int route_report(char* buf, int len) {
  std::string out;
  for (auto& l : g_route_lines) { out += l; out += "\n"; }
  if (buf && len > 0) { strncpy(buf, out.c_str(), len - 1); buf[len - 1] = 0; }
  return (int)out.size();
}

// ---------------------------------------------------------------------------------------
Ctx::Ctx(void* stream, size_t ws_bytes) {
  s.handle = stream;
  s.ws_bytes = ws_bytes;
  s.ws = static_cast<char*>(dev_alloc(ws_bytes));
}
Ctx::Ctx(const Stream& shared) : s(shared), owns_ws(false) {}
Ctx::~Ctx() {
  // nothing may still be running on a stream whose events and handle are about to be destroyed (round-4 advice)
  try {
    if (owned_comm_stream) stream_sync(comm_stream);
    if (has_side) stream_sync(side);
  } catch (...) {}
  release(allocs);
  if (owns_ws) dev_free(s.ws);
  if (owned_comm_stream) {
    for (void* e : comm_events) event_destroy(e);
    event_destroy(comm_join_event);
    stream_destroy(owned_comm_stream);
  }
  if (has_side) {
    dev_free(side.ws);
    for (void* e : fork_events) event_destroy(e);
    event_destroy(join_event);
    stream_destroy(owned_side_stream);
  }
}
void Ctx::enable_side(int device) {
  if (has_side || !is_device_build()) return;
  owned_side_stream = stream_create(device);
  side.handle = owned_side_stream;
  side.ws_bytes = s.ws_bytes;
  side.ws = static_cast<char*>(dev_alloc(side.ws_bytes));
  for (int i = 0; i < 8; ++i) fork_events.push_back(event_create());
  join_event = event_create();
  has_side = true;
}
Stream& Ctx::fork_side() {
  void* ev = fork_events[fork_i++ % fork_events.size()];
  event_record(ev, s);
  stream_wait_event(side, ev);
  side_dirty = true;
  return side;
}
void Ctx::join_side() {
  if (!has_side || !side_dirty) return;
  event_record(join_event, side);
  stream_wait_event(s, join_event);
  side_dirty = false;
}
void Ctx::attach_comm(AllReduceFn fn, void* comm, int world) {
  comm_join();
  if (!fn) {
    // detaching: the caller is about to destroy the communicator -- no collective of ours may still be in flight on its stream
    if (owned_comm_stream) stream_sync(comm_stream);
    comm_fn = nullptr; comm_handle = nullptr; comm_world = 1;
    return;
  }
  if (world < 1) throw Error(1, "attach_comm: world size must be >= 1");
  comm_fn = fn; comm_handle = comm; comm_world = world;
  if (is_device_build() && !owned_comm_stream) {
    owned_comm_stream = stream_create(device_index);
    comm_stream.handle = owned_comm_stream;       // no scratch: nothing launched there uses the split-K workspace
    for (int i = 0; i < 8; ++i) comm_events.push_back(event_create());
    comm_join_event = event_create();
  }
}
Stream& Ctx::comm_fork() {
  if (!owned_comm_stream) return s;               // host simulator: one in-order stream
  void* ev = comm_events[comm_ev_i++ % comm_events.size()];
  event_record(ev, s);
  stream_wait_event(comm_stream, ev);
  comm_dirty = true;
  return comm_stream;
}
void Ctx::comm_join() {
  if (!owned_comm_stream || !comm_dirty) return;
  event_record(comm_join_event, comm_stream);
  stream_wait_event(s, comm_join_event);
  comm_dirty = false;
}
void Ctx::all_reduce_sum(Stream& on, float* buf, size_t count) {
  if (!comm_fn) throw Error(1, "all_reduce: no communicator attached (swn_ctx_attach_comm)");
  if (count == 0) return;
  // ncclFloat32 = 7, ncclSum = 0 (nccl.h / rccl.h)
  const int rc = comm_fn(buf, buf, count, 7, 0, comm_handle, on.handle);
  if (rc != 0) throw Error(2, "all_reduce: the attached all-reduce returned " + std::to_string(rc));
}
void* Ctx::alloc(size_t bytes) {
  void* p = dev_alloc(bytes);
  (sink ? *sink : allocs).push_back({p, bytes});
  bytes_allocated += bytes;
  return p;
}
void Ctx::release(AllocList& list) {
  for (auto& a : list) { dev_free(a.first); bytes_allocated -= a.second; }
  list.clear();
}
Model::~Model() {
  for (void*& g : step_graph_) { graph_destroy(g); g = nullptr; }
  if (cap_stream_) stream_destroy(cap_stream_);
  gp_.reset(); D3_.reset(); G.reset(); D2.reset(); D1.reset();
  if (ctx) ctx->release(owned_allocs);
}

Var Var::slice(int c0, int c) const {
  Var r = *this;
  r.v = v.slice(c0, c);
  if (has_grad) r.g = g.slice(c0, c);
  return r;
}
Var Var::batch(int n0, int n) const {
  Var r = *this;
  const size_t off = (size_t)n0 * v.H * v.W * v.cs;
  r.v.p = v.p + off; r.v.N = n;
  if (has_grad) { r.g.p = g.p + off; r.g.N = n; }
  return r;
}

// ---------------------------------------------------------------------------------------
int ParamArena::add_weight(const std::string& name, int kind, int Co, int Ci, int KH, int KW, int Cip,
                           const std::vector<int32_t>* cimap) {
  if (frozen) {
    auto it = index.find(name);
    if (it == index.end()) throw Error(1, "shared arena has no parameter " + name);
    const WShape& e = params[it->second].ws;
    if (e.kind != kind || e.Co != Co || e.Ci != Ci || e.KH != KH || e.KW != KW || e.Cip != Cip)
      throw Error(1, "shared arena: shape mismatch for " + name);
    return it->second;
  }
  ParamDesc d;
  d.name = name;
  d.ws.kind = kind; d.ws.Co = Co; d.ws.Ci = Ci; d.ws.KH = KH; d.ws.KW = KW; d.ws.Cip = Cip;
  d.ws.Npad = round_up(Co, 4);
  if (cimap) d.cimap = *cimap;
  d.elems = packed_elems(d.ws);
  d.off = n;
  n += (d.elems + 3) / 4 * 4;
  index[name] = (int)params.size();
  params.push_back(d);
  return (int)params.size() - 1;
}
int ParamArena::add_bias(const std::string& name, int nb) {
  if (frozen) {
    auto it = index.find(name);
    if (it == index.end() || params[it->second].n_logical != nb) throw Error(1, "shared arena: bad bias " + name);
    return it->second;
  }
  ParamDesc d;
  d.name = name; d.is_bias = true; d.n_logical = nb;
  d.elems = round_up(nb, 4);
  d.off = n;
  n += d.elems;
  index[name] = (int)params.size();
  params.push_back(d);
  return (int)params.size() - 1;
}
void ParamArena::allocate(Ctx& c) {
  const size_t bytes = std::max<size_t>(n, 4) * sizeof(float);
  w = static_cast<float*>(c.alloc(bytes));
  g = static_cast<float*>(c.alloc(bytes));
  m = static_cast<float*>(c.alloc(bytes));
  v = static_cast<float*>(c.alloc(bytes));
  for (auto& d : params) {
    if (!d.cimap.empty()) {
      int32_t* dev = static_cast<int32_t*>(c.alloc(d.cimap.size() * sizeof(int32_t)));
      dev_upload(c.s, dev, d.cimap.data(), d.cimap.size() * sizeof(int32_t));
      d.ws.cimap = dev;
    }
  }
  frozen = true;
}

// ---------------------------------------------------------------------------------------
Var Net::alloc_var(int N, int H, int W, int C, bool need_grad) {
  if (C % 4) throw Error(1, "alloc_var: C must be a multiple of 4");
  Var r;
  const size_t bytes = (size_t)N * H * W * C * sizeof(float);
  r.v.p = static_cast<float*>(ctx.alloc(bytes));
  r.v.N = N; r.v.H = H; r.v.W = W; r.v.C = C; r.v.cs = C;
  r.vbase = r.v.p;
  r.has_grad = need_grad;
  if (need_grad) {
    r.g = r.v;
    r.g.p = static_cast<float*>(ctx.alloc(bytes));
    r.gbase = r.g.p;
  }
  return r;
}

size_t Net::reserve_dg(Op* op, size_t elems) {
  const size_t off = dg_n;
  dg_n += (elems + 3) / 4 * 4;
  dg_layout.push_back({op, off});
  return off;
}

namespace {
struct ConvGeom {
  Gather fwd;       // forward gather (Ho,Wo filled)
  int Ho = 0, Wo = 0;
};
ConvGeom conv_geom(ConvKind kind, int H, int W) {
  ConvGeom c;
  Gather& g = c.fwd;
  switch (kind) {
    case CK_K4S2: g.KH = g.KW = 4; g.stride = 2; g.pad_t = g.pad_l = 1; c.Ho = H / 2; c.Wo = W / 2; break;
    case CK_K3S1_REFLECT: g.KH = g.KW = 3; g.stride = 1; g.pad_t = g.pad_l = 1; g.pad_mode = PAD_REFLECT; c.Ho = H; c.Wo = W; break;
    case CK_K3S1_ZERO: g.KH = g.KW = 3; g.stride = 1; g.pad_t = g.pad_l = 1; c.Ho = H; c.Wo = W; break;
    case CK_K4S1: g.KH = g.KW = 4; g.stride = 1; g.pad_t = g.pad_l = 1; c.Ho = H - 1; c.Wo = W - 1; break;
    case CK_K1S1: g.KH = g.KW = 1; g.stride = 1; g.pad_t = g.pad_l = 0; c.Ho = H; c.Wo = W; break;
    case CK_TAIL_UP:   // Upsample(x2) + ZeroPad2d((1,0,1,0)) + Conv(k4,p1): pad 2 top/left in upsampled coords
      g.KH = g.KW = 4; g.stride = 1; g.pad_t = g.pad_l = 2; g.ups = 1; c.Ho = H * 2; c.Wo = W * 2; break;
  }
  g.Ho = c.Ho; g.Wo = c.Wo;
  return c;
}

// The Winograd switches, read when a layer is built (tests toggle them between layers): Net::conv / Net::convT read them once
// and hand them to the route predicates below
struct WinoSwitches {
  bool on, s2_on;       // SWN_WINOGRAD, SWN_WINO_S2: off when 0
  int minc, force_m;    // SWN_WINO_MINC > 0: the channel threshold of every form (tests: small channel counts too); SWN_WINO_M
};
WinoSwitches wino_switches() {
  return {env_on(getenv("SWN_WINOGRAD")), env_on(getenv("SWN_WINO_S2")), env_int(getenv("SWN_WINO_MINC"), 0), env_int(getenv("SWN_WINO_M"), 0)};
}

// ---- strided Winograd F(4x4, 2x2) for the k4 s2 p1 convolutions and their transposes (ops.h wino_s2_*, wino.hip) ----------
// Used where the activation side dominates: the transformed filters are 6.25x the weights (per GEMM direction) and are
// re-derived every optimizer step, so the 8-16 M-parameter layers at 4x4 / 8x8 maps stay on the direct kernels.
bool s2_wino_wanted(const WinoSwitches& sw, int Cfine, int Ccoarse, int Hc, int Wc) {
  if (!sw.on || !sw.s2_on) return false;
  const int minc = sw.minc > 0 ? sw.minc : 256;
  if (Ccoarse < minc || Cfine < 32 || Cfine % 4 || Ccoarse % 16 || Hc < 2 || Wc < 2) return false;
  // coarse maps of at least 16 x 16: below that the GEMMs are a handful of tiles (nothing to gain), and the 8 x 8 ... 2 x 2
  // levels of the pix2pix U-Net sit in front of InstanceNorms over 64 ... 4 pixels, which amplify the (2.5x larger) round-off
  // of the Winograd form: with them on it, the texture generator's gradients were 1e-4 ... 3e-4 off the pinned float64 oracle,
  // without 6e-5 (tests/test_pattern_replay.py)
  if (sw.minc <= 0 && Hc * Wc < 256) return false;
  return (size_t)16 * Cfine * Ccoarse <= ((size_t)1 << 22);
}

// Stride-1 convs with MFMA-friendly channel counts run as Winograd F(m x m, r x r): transform,
// (m+r-1)^2 batched GEMMs, inverse transform (wino.hip).  3x3: F(4x4,3x3) when H and W are
// multiples of 4 (4x fewer multiplies), else F(2x2,3x3) (2.25x); PatchGAN's k4 s1: F(3x3,4x4) (4x).
// ... when the channel counts are large enough for the GEMMs (K = Cin each) to run at MFMA speed
// and to amortise the HBM-bound transforms: measured on VGG16 (texture C3), the 6-point forms win
// from 64 channels up, F(2x2,3x3) (4x instead of 2.25x transform data per input) only from 256.
// Returns m, 0 = the layer stays on the direct kernels.
int wino_s1_m(const WinoSwitches& sw, ConvKind kind, int Cip, int Co, int H, int W) {
  const bool is_k3 = kind == CK_K3S1_REFLECT || kind == CK_K3S1_ZERO, is_k4 = kind == CK_K4S1;
  const int wm = is_k4 ? 3 : ((sw.force_m != 2 && H % 4 == 0 && W % 4 == 0) ? 4 : 2);
  const int minc = sw.minc > 0 ? sw.minc : (wm == 2 ? 256 : 64);
  const bool wino = sw.on && Cip % 32 == 0 && Co % 32 == 0 && Cip >= minc && Co >= minc && H >= 4 && W >= 4 &&
                    ((is_k3 && H % 2 == 0 && W % 2 == 0) || is_k4);
  return wino ? wm : 0;
}

// ---- the batched GEMMs over Winograd planes: P planes of T rows each ---------------------------------------------------------
TView plane_mat(float* p, size_t T, int C) {
  TView v; v.p = p; v.N = 1; v.H = 1; v.W = (int)T; v.C = C; v.cs = C; return v;     // T x C matrix
}
// How a GEMM learns the scale of a plane operand: the exponent its producer stored it in pair form with (ops.h
// wino_input_transform), or the planes' amax slot, or neither (fp32 planes without a slot: the launch takes the amax itself)
struct PlaneScale { const int* pair_k = nullptr; const float* amax = nullptr; };
PlaneScale plane_scale(bool pairs, const int* k, const float* amax) { return pairs ? PlaneScale{k, nullptr} : PlaneScale{nullptr, amax}; }
// The [K x N] panels: fp32 (NULL where the panel exists only pre-cut) and / or pre-cut for column tile `tile` (0 = none), `bs`
// elements between planes
struct PlanePanel { const float* w; const uint16_t* pc; int tile; size_t bs; };
// P planes of [T x K] . [K x N] -> [T x N]
ConvFwdArgs plane_gemm(float* x, float* y, size_t T, int K, int N, int Cout, int P, PlaneScale xs, PlanePanel w) {
  ConvFwdArgs g;
  g.x = plane_mat(x, T, K); g.g.Ho = 1; g.g.Wo = (int)T;
  g.w = w.w; g.Npad = N; g.Cout = Cout;
  g.y = plane_mat(y, T, N);
  g.batch = P; g.x_bs = T * K; g.w_bs = (size_t)K * N; g.y_bs = T * N;
  g.x_pair_k = xs.pair_k; g.x_amax = xs.amax;
  if (w.tile) { g.wpc = w.pc; g.wpc_bn = w.tile; g.wpc_bs = w.bs; }
  return g;
}
// P planes of [T x K]^T . [T x N] -> [K x N]
ConvWgradArgs plane_wgrad(float* x, float* dy, float* dw, size_t T, int K, int N, int Cout, int P, PlaneScale xs, PlaneScale dys) {
  ConvWgradArgs g;
  g.x = plane_mat(x, T, K); g.g.Ho = 1; g.g.Wo = (int)T;
  g.dy = plane_mat(dy, T, N);
  g.dw = dw; g.Npad = N; g.Cout = Cout;
  g.batch = P; g.x_bs = T * K; g.dy_bs = T * N; g.dw_bs = (size_t)K * N;
  g.x_pair_k = xs.pair_k; g.x_amax = xs.amax;
  g.dy_pair_k = dys.pair_k; g.dy_amax = dys.amax;
  return g;
}

// Column tile of a pre-cut operand written by the 6-point FILTER TRANSFORM (ops.h wino_filter_transform_pc): that kernel lays out
// tiles of 64 or 128 columns only.  conv_precut_tile answers 192 for widths in (128, 192] (the tile of the tail conv's input
// gradient, produced by conv_precut) -- a stride-1 Winograd layer of such a width keeps its fp32 U and the kernels that read it,
// and with them fp32 planes: planning and launch agree instead of failing at the first operand refresh (latent: no network of
// the reference has a 3x3 / 4x4 stride-1 conv between 129 and 192 channels; swn_op_conv can ask for one).
int wino_precut_tile(int xC, int Npad) {
  const int t = conv_precut_tile(xC, Npad);
  return (t == 64 || t == 128) ? t : 0;
}
bool wino_fwd_takes_pairs(int xC, int Npad) { return wino_precut_tile(xC, Npad) != 0 && conv_fwd_takes_pairs(xC, Npad); }

bool bias_on_main() { static const bool on = env_on(getenv("SWN_BIAS_MAIN")); return on; }
}  // namespace

// What every route builder of a layer needs (Net::conv / Net::convT fill it; it lives for the builder's call only, so the
// closures copy what they keep).  convT: kind / Ci / actf / geo / x_is_input / dgrad_C are not used.
struct Net::ConvLayer {
  const std::string& name;
  const Var &x, &y;
  ConvKind kind;
  int Ci, Co, Cip, Cop;     // logical and buffer channels of input and output
  int wi, bi;               // arena entries of weight and bias (bi < 0: none)
  int actf;
  ConvGeom geo;
  bool x_is_input;
  int dgrad_C;
};

// ---- Conv2d ---------------------------------------------------------------------------
// y.v receives act(conv(x)+bias).  In backward y.g is the gradient w.r.t. that output.
void Net::conv(const std::string& name, const Var& x, const Var& y, ConvKind kind, int Ci, int Co, bool bias,
               int actf, const std::vector<int32_t>* cimap, bool x_is_input, int dgrad_C) {
  const WinoSwitches sw = wino_switches();
  const int KH = kind == CK_K1S1 ? 1 : ((kind == CK_K3S1_REFLECT || kind == CK_K3S1_ZERO) ? 3 : 4);
  const ConvGeom geo = conv_geom(kind, x.v.H, x.v.W);
  if (y.v.H != geo.Ho || y.v.W != geo.Wo) throw Error(1, "conv " + name + ": output view has the wrong size");
  const int Cip = x.v.C;
  if (Ci > Cip) throw Error(1, "conv " + name + ": Ci exceeds the input view's channels");
  const int wi = arena.add_weight(name + ".weight", WK_CONV, Co, Ci, KH, KH, Cip, cimap);
  const int bi = bias ? arena.add_bias(name + ".bias", Co) : -1;
  const int Cop = round_up(Co, 4);
  if (y.v.C != Cop) throw Error(1, "conv " + name + ": output view must have round_up(Co,4) channels");
  note_act(actf, y.v);

  auto op = std::make_unique<Op>();
  op->label = name;
  op->param_off = arena.params[wi].off;
  op->reads_net_input = x_is_input;
  const ConvLayer L{name, x, y, kind, Ci, Co, Cip, Cop, wi, bi, actf, geo, x_is_input, dgrad_C};
  // PatchGAN's 1-channel head conv (discriminators.py:131): taps on the N axis (ops.h head_*): the input
  // is read once by a 1x1 conv with N = 16 instead of 16 times by an N = 1 implicit GEMM.
  if (env_on(getenv("SWN_HEAD_TAPN")) && kind == CK_K4S1 && Co == 1 && Cip % 32 == 0 && actf == ACT_NONE && x.has_grad == y.has_grad)
    conv_head_tapn(L, *op);
  // k4 s2 convs with enough channels: strided Winograd F(4x4,2x2) (four polyphase 2x2 convolutions in one batched GEMM)
  // (never the layers that read a network input: their buffers carry layout pad channels -- 19 -> 32, 22 -> 32 -- that would
  // be transformed for nothing, and the channel threshold of the test routing must not reach them through the padding)
  else if (kind == CK_K4S2 && s2_wino && !x_is_input && s2_wino_wanted(sw, Cip, Cop, y.v.H, y.v.W) && Co % 4 == 0)
    conv_wino_s2(L, *op);
  // The tail conv in Winograd form (ops.h tailw_*): the four folded sub-pixel phases share one F(4x4,3x3) input transform of the
  // un-upsampled map and one batched GEMM with N = 4 Npad; forward and weight gradient (the input gradient stays the folded
  // 5x5 stride-2 conv on the ring kernel: its Winograd form would be bound by the adjoint transform of a 0.9 GB operand)
  else if (kind == CK_TAIL_UP && sw.on && Cip % 32 == 0 && Cip >= (sw.minc > 0 ? sw.minc : 64) && x.v.H >= 4 && x.v.W >= 4 && Cop <= 32)
    conv_tail_wino(L, *op);
  else if (const int wm = wino_s1_m(sw, kind, Cip, Co, x.v.H, x.v.W))
    conv_wino_s1(L, wm, *op);
  else
    conv_direct(L, *op);
  ops.push_back(std::move(op));
}

void Net::conv_head_tapn(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const int Cip = L.Cip, wi = L.wi, bi = L.bi;
  ParamArena* A = &arena; Op* self = &op;
  const TView xv = x.v, yv = y.v;
  const size_t wt_off = reserve_dg(self, (size_t)Cip * 16), wt2_off = reserve_dg(self, (size_t)16 * Cip);
  const size_t dwt_off = reserve_dg(self, (size_t)Cip * 16);
  note_writer(y.vbase, false);
  Var Z = alloc_var(xv.N, xv.H, xv.W, 16, false);          // Z forward, dZ backward (same scratch)
  const TView zv = Z.v, ygv = y.g, xgv = x.g;
  const bool has_grad = y.has_grad;
  op.repack = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    head_pack(n.ctx.s, wd.ws, A->w + wd.off, n.dg + wt_off, n.dg + wt2_off);
  };
  op.fwd = [=](Net& n) {
    n.need(self);
    ConvFwdArgs a;
    a.x = xv; a.g.Ho = xv.H; a.g.Wo = xv.W;               // 1x1, stride 1
    a.w = n.dg + wt_off; a.Npad = 16; a.Cout = 16; a.y = zv;
    conv_fwd(n.ctx.s, a);
    head_gather(n.ctx.s, zv, bi >= 0 ? A->w + A->params[bi].off : nullptr, yv);
  };
  if (has_grad) op.grad_targets.push_back(x);
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_grad) return;
    const ParamDesc& wd = A->params[wi];
    head_scatter(n.ctx.s, ygv, zv);
    if (wgrad) {
      Stream& sw = n.wgrad_stream();
      ConvWgradArgs wa;
      wa.x = xv; wa.g.Ho = xv.H; wa.g.Wo = xv.W; wa.dy = zv;
      wa.dw = n.dg + dwt_off; wa.Npad = 16; wa.Cout = 16;
      conv_wgrad(sw, wa);
      head_unpack_grad(sw, wd.ws, n.dg + dwt_off, A->g + wd.off);
      if (bi >= 0) n.bias_grad_of(sw, ygv, A->g + A->params[bi].off);
    }
    if (me.reads_net_input && !igrad) return;
    ConvFwdArgs d;
    d.x = zv; d.g.Ho = xv.H; d.g.Wo = xv.W;
    d.w = n.dg + wt2_off; d.Npad = Cip; d.Cout = Cip; d.y = xgv; d.accumulate = me.acc.empty() ? 0 : me.acc[0];
    conv_fwd(n.ctx.s, d);
  };
}

void Net::conv_wino_s2(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const int Co = L.Co, Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi, actf = L.actf;
  ParamArena* A = &arena; Op* self = &op;
  const TView xv = x.v, yv = y.v;
  const int sP = 25, sTh = ceil_div(y.v.H, 4), sTw = ceil_div(y.v.W, 4), CV = 4 * Cip;
  const size_t sT = (size_t)x.v.N * sTh * sTw;
  const bool want_dx = x.has_grad && y.has_grad;
  const size_t uf_off = reserve_dg(self, (size_t)sP * CV * Cop);                      // U  [25][4 Cip][Cop]
  const size_t ut_off = want_dx ? reserve_dg(self, (size_t)sP * Cop * CV) : 0;        // U^T[25][Cop][4 Cip]
  float* keepV = (keep_wino_inputs && y.has_grad) ? static_cast<float*>(ctx.alloc(sP * sT * CV * sizeof(float))) : nullptr;
  wsV_need = std::max(wsV_need, sP * sT * (size_t)std::max(CV, Cop));
  wsM_need = std::max(wsM_need, sP * sT * (size_t)std::max(CV, Cop));
  wsU_need = std::max(wsU_need, (size_t)sP * CV * Cop);
  const int pcf = conv_precut_tile(CV, Cop), pct = want_dx ? conv_precut_tile(Cop, CV) : 0;
  const size_t pcf_bs = pcf ? conv_precut_elems(CV, Cop, pcf) : 0, pct_bs = pct ? conv_precut_elems(Cop, CV, pct) : 0;
  const size_t pcf_off = pcf ? reserve_dgp(pcf_bs * sP) : 0, pct_off = pct ? reserve_dgp(pct_bs * sP) : 0;
  const size_t slV = reserve_slot(), slD = reserve_slot();      // amax of V (forward planes) and of dM (transformed dY)
  note_writer(y.vbase, false);
  // pair-form planes (ops.h wino_input_transform) where every GEMM that reads them takes the kernels that can, and -- decided
  // per pass -- the transform's input has a complete amax slot to bound the planes with
  const bool pairV_ok = conv_fwd_takes_pairs(CV, Cop) && (!y.has_grad || conv_wgrad_takes_pairs(sT, CV, Cop));
  const bool pairD_ok = conv_wgrad_takes_pairs(sT, CV, Cop) && (!(x.has_grad && y.has_grad) || conv_fwd_takes_pairs(Cop, CV));
  const size_t kV = reserve_k(), kD = reserve_k();
  const float* xbase = x.vbase; const float* ygbase = y.gbase;
  // dM = A dY A^T serves the weight gradient (side stream) and the input gradient (main stream): one buffer per layer
  float* keepdM = (y.has_grad && want_dx && share_dy()) ? static_cast<float*>(ctx.alloc(sP * sT * Cop * sizeof(float))) : nullptr;
  op.repack = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    const float* wmax = nullptr;       // U^T holds U's values: one amax pass serves both operands (ops.h conv_precut amax_io)
    wino_s2_filter_transform(n.ctx.s, wd.ws, 0, A->w + wd.off, n.dg + uf_off);
    if (pcf) conv_precut(n.ctx.s, n.dg + uf_off, CV, Cop, pcf, sP, (size_t)CV * Cop, n.dgp + pcf_off, &wmax);
    if (want_dx) {
      wino_s2_filter_transform(n.ctx.s, wd.ws, 1, A->w + wd.off, n.dg + ut_off);
      if (pct) conv_precut(n.ctx.s, n.dg + ut_off, Cop, CV, pct, sP, (size_t)Cop * CV, n.dgp + pct_off, &wmax);
    }
  };
  op.fwd = [=](Net& n) {
    n.need(self);
    float* V = keepV ? keepV : n.wsV;
    const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
    wino_s2_input_transform(n.ctx.s, xv, sTh, sTw, V, n.amax + slV, xin, n.kscale + kV);
    conv_fwd(n.ctx.s, plane_gemm(V, n.wsM, sT, CV, Cop, Co, sP, plane_scale(xin != nullptr, n.kscale + kV, n.amax + slV),
                                 {n.dg + uf_off, n.dgp + pcf_off, pcf, pcf_bs}));
    wino_output_transform(n.ctx.s, 4, 2, n.wsM, Cop, sTh, sTw, bi >= 0 ? A->w + A->params[bi].off : nullptr, actf, yv, Co, 0);
  };
  Var scratch;
  if (y.has_grad && actf != ACT_NONE) scratch = alloc_var(yv.N, yv.H, yv.W, Cop, false);
  if (want_dx) op.grad_targets.push_back(x);
  const TView ygv = y.g, xgv = x.g, scr = scratch.v;
  const bool has_ygrad = y.has_grad;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    TView dY = ygv;
    // (a fused activation's dR has no amax slot in this branch: its planes stay fp32 and the GEMM takes their amax)
    if (actf != ACT_NONE) { act_bwd(n.ctx.s, ygv, yv, scr, actf, 0); dY = scr; }
    const ParamDesc& wd = A->params[wi];
    const bool dx_now = want_dx && !(me.reads_net_input && !igrad);
    const bool shared = keepdM && wgrad && dx_now;       // one transform of dY on the main stream, read by both gradients
    const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
    const float* din = (pairD_ok && actf == ACT_NONE) ? n.slot_if_complete(ygbase) : nullptr;
    const PlaneScale dMs = plane_scale(din != nullptr, n.kscale + kD, n.amax + slD);
    if (shared) wino_dy_transform(n.ctx.s, 4, 2, dY, sTh, sTw, keepdM, n.amax + slD, din, n.kscale + kD);
    if (wgrad) {
      Stream& sw = n.wgrad_stream();
      float* V = keepV ? keepV : n.wsV;
      float* dM = shared ? keepdM : n.wgrad_planes(sw);
      if (!keepV) wino_s2_input_transform(sw, xv, sTh, sTw, V, n.amax + slV, xin, n.kscale + kV);
      if (!shared) wino_dy_transform(sw, 4, 2, dY, sTh, sTw, dM, n.amax + slD, din, n.kscale + kD);
      conv_wgrad(sw, plane_wgrad(V, dM, n.wsU, sT, CV, Cop, Co, sP, plane_scale(xin != nullptr, n.kscale + kV, n.amax + slV), dMs));
      wino_s2_filter_grad(sw, wd.ws, n.wsU, A->g + wd.off);
      if (bi >= 0) n.bias_grad_of(sw, dY, A->g + A->params[bi].off);
    }
    if (!dx_now) return;
    float* dMx = shared ? keepdM : n.wsV;
    if (!shared) wino_dy_transform(n.ctx.s, 4, 2, dY, sTh, sTw, dMx, n.amax + slD, din, n.kscale + kD);
    conv_fwd(n.ctx.s, plane_gemm(dMx, n.wsM, sT, Cop, CV, CV, sP, dMs, {n.dg + ut_off, n.dgp + pct_off, pct, pct_bs}));
    wino_s2_input_adjoint(n.ctx.s, n.wsM, Cip, sTh, sTw, xgv, nullptr, me.acc.empty() ? 0 : me.acc[0]);
  };
}

void Net::conv_tail_wino(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const int Co = L.Co, Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi, actf = L.actf;
  ParamArena* A = &arena; Op* self = &op;
  const TView xv = x.v, yv = y.v;
  const ParamDesc wd0 = arena.params[wi];
  const int tP = 36, tTh = ceil_div(x.v.H, 4), tTw = ceil_div(x.v.W, 4), N4 = 4 * Cop;
  const size_t tT = (size_t)x.v.N * tTh * tTw;
  const size_t fe = tail_fold_offset(wd0.ws, 4);
  const size_t fold_off = reserve_dg(self, fe), dfold_off = reserve_dg(self, fe);
  const size_t tu_off = reserve_dg(self, (size_t)tP * Cip * N4);
  float* keepV = (keep_wino_inputs && y.has_grad) ? static_cast<float*>(ctx.alloc(tP * tT * Cip * sizeof(float))) : nullptr;
  wsV_need = std::max(wsV_need, tP * tT * (size_t)std::max(Cip, N4));
  wsM_need = std::max(wsM_need, tP * tT * (size_t)std::max(Cip, N4));
  wsU_need = std::max(wsU_need, (size_t)tP * Cip * N4);
  const int pcu = conv_precut_tile(Cip, N4);
  const size_t pcu_bs = pcu ? conv_precut_elems(Cip, N4, pcu) : 0, pcu_off = pcu ? reserve_dgp(pcu_bs * tP) : 0;
  const size_t slV = reserve_slot(), slD = reserve_slot();
  note_writer(y.vbase, false);
  const bool pairV_ok = conv_fwd_takes_pairs(Cip, N4) && (!y.has_grad || conv_wgrad_takes_pairs(tT, Cip, N4));
  const bool pairD_ok = conv_wgrad_takes_pairs(tT, Cip, N4);
  const size_t kV = reserve_k(), kD = reserve_k();
  const float* xbase = x.vbase;
  // input gradient: the folded 5x5 stride-2 conv over dR (32-channel buffer, see CopD in conv_direct)
  const bool want_dx = x.has_grad && y.has_grad;
  const int CopD = (actf != ACT_NONE && want_dx && conv_precut_tile(32, Cip) == 192) ? 32 : Cop;
  const size_t dg_off = want_dx ? reserve_dg(self, dgrad_elems(wd0.ws, 3, CopD, Cip)) : 0;
  const int pc_d = want_dx ? conv_precut_tile(CopD, Cip) : 0;
  const size_t pcd_bs = pc_d ? conv_precut_elems(25 * CopD, Cip, pc_d) : 0, pcd_off = pc_d ? reserve_dgp(pcd_bs) : 0;
  op.repack = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    tail_fold_weights(n.ctx.s, wd.ws, A->w + wd.off, n.dg + fold_off);
    tailw_filter_transform(n.ctx.s, wd.ws, n.dg + fold_off, n.dg + tu_off);
    if (pcu) conv_precut(n.ctx.s, n.dg + tu_off, Cip, N4, pcu, tP, (size_t)Cip * N4, n.dgp + pcu_off);
    if (want_dx) {
      repack_dgrad(n.ctx.s, wd.ws, 3, CopD, Cip, A->w + wd.off, n.dg + dg_off);
      if (pc_d) conv_precut(n.ctx.s, n.dg + dg_off, 25 * CopD, Cip, pc_d, 1, 0, n.dgp + pcd_off);
    }
  };
  op.fwd = [=](Net& n) {
    n.need(self);
    float* V = keepV ? keepV : n.wsV;
    const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
    wino_input_transform(n.ctx.s, 4, 3, xv, 1, PAD_ZERO, tTh, tTw, V, n.amax + slV, xin, n.kscale + kV);
    conv_fwd(n.ctx.s, plane_gemm(V, n.wsM, tT, Cip, N4, N4, tP, plane_scale(xin != nullptr, n.kscale + kV, n.amax + slV),
                                 {n.dg + tu_off, n.dgp + pcu_off, pcu, pcu_bs}));
    tailw_output_transform(n.ctx.s, n.wsM, tTh, tTw, Cop, bi >= 0 ? A->w + A->params[bi].off : nullptr, actf, yv, Co);
  };
  Var scratch;
  if (y.has_grad && actf != ACT_NONE) scratch = alloc_var(yv.N, yv.H, yv.W, CopD, false);
  if (want_dx) op.grad_targets.push_back(x);
  const TView ygv = y.g, xgv = x.g, scr = CopD != Cop ? scratch.v.slice(0, Cop) : scratch.v, scr_full = scratch.v;
  const bool has_ygrad = y.has_grad;
  const size_t scrSlot = (y.has_grad && actf != ACT_NONE) ? note_writer(scratch.v.p, true) : 0;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    TView dY = ygv;
    const float* dy_slot = nullptr;
    if (actf != ACT_NONE) { act_bwd(n.ctx.s, ygv, yv, scr, actf, 0, n.amax + scrSlot); dY = scr; dy_slot = n.amax + scrSlot; }
    const ParamDesc& wd = A->params[wi];
    if (wgrad) {
      Stream& sw = n.wgrad_stream();
      float* V = keepV ? keepV : n.wsV;
      float* dM = n.wgrad_planes(sw);
      const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
      const float* din = pairD_ok ? dy_slot : nullptr;
      if (!keepV) wino_input_transform(sw, 4, 3, xv, 1, PAD_ZERO, tTh, tTw, V, n.amax + slV, xin, n.kscale + kV);
      tailw_dy_transform(sw, dY, tTh, tTw, Cop, dM, n.amax + slD, din, n.kscale + kD);
      conv_wgrad(sw, plane_wgrad(V, dM, n.wsU, tT, Cip, N4, N4, tP, plane_scale(xin != nullptr, n.kscale + kV, n.amax + slV),
                                 plane_scale(din != nullptr, n.kscale + kD, n.amax + slD)));
      tailw_filter_grad(sw, wd.ws, n.wsU, n.dg + dfold_off);
      tail_unfold_wgrad(sw, wd.ws, n.dg + dfold_off, A->g + wd.off);
      if (bi >= 0) n.bias_grad_of(sw, dY, A->g + A->params[bi].off);
    }
    if (!want_dx || (me.reads_net_input && !igrad)) return;
    ConvFwdArgs d;
    d.x = CopD != Cop ? scr_full : dY;
    d.g.KH = d.g.KW = 5; d.g.stride = 2; d.g.pad_t = d.g.pad_l = 1; d.g.Ho = xv.H; d.g.Wo = xv.W;
    d.w = n.dg + dg_off; d.Npad = Cip; d.Cout = Cip; d.y = xgv; d.accumulate = me.acc.empty() ? 0 : me.acc[0];
    d.x_amax = dy_slot;
    if (pc_d) { d.wpc = n.dgp + pcd_off; d.wpc_bn = pc_d; d.wpc_bs = pcd_bs; }
    conv_fwd(n.ctx.s, d);
  };
}

// Stride-1 Winograd F(wm x wm, r x r), r from the kernel size (the predicate and its reasons: wino_s1_m)
void Net::conv_wino_s1(const ConvLayer& L, int wm, Op& op) {
  const Var &x = L.x, &y = L.y;
  const ConvKind kind = L.kind;
  const int Co = L.Co, Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi, actf = L.actf;
  ParamArena* A = &arena; Op* self = &op;
  const Gather gf = L.geo.fwd;
  const TView xv = x.v, yv = y.v;
  const int wr = kind == CK_K4S1 ? 4 : 3;
  const int wP = (wm + wr - 1) * (wm + wr - 1);
  const int wTh = ceil_div(y.v.H, wm), wTw = ceil_div(y.v.W, wm);
  const size_t wT = (size_t)x.v.N * wTh * wTw;
  // dgrad of the REFLECT-padded convs (the resblocks) = the adjoint of the forward Winograd pipeline, in the forward tiling:
  // dV = (A dY A^T) U^T, dx = adjoint input transform (ops.h wino_input_adjoint) -- 16 tiles per 16x16 map where the
  // transposed-conv form walks the 18x18 padded gradient grid in 25.  The zero-padded convs (VGG16, PatchGAN's k4 s1)
  // keep the transposed stride-1 conv over dY (pad r-1-p, tiles over the input grid): same tile count either way, and it is the
  // better-conditioned form (its large-entry matrices B^T / A^T act on data, not on the GEMM's output).
  const bool wadj = kind == CK_K3S1_REFLECT;
  const int wpad2 = kind == CK_K3S1_ZERO ? 1 : 2;
  const int wTh2 = ceil_div(x.v.H, wm), wTw2 = ceil_div(x.v.W, wm);
  const size_t wT2 = wadj ? 0 : (size_t)x.v.N * wTh2 * wTw2;
  // V = B^T d B of the forward input, reused by the weight gradient
  float* keepV = (keep_wino_inputs && y.has_grad) ? static_cast<float*>(ctx.alloc((size_t)wP * wT * Cip * sizeof(float))) : nullptr;
  // 6-point forms: the transformed filters go straight into the pre-cut operand layout of the ring kernel (no fp32 U)
  const int pcw = wm != 2 ? wino_precut_tile(Cip, Cop) : 0;
  const size_t pcw_bs = pcw ? conv_precut_elems(Cip, Cop, pcw) : 0;
  // amax slots of the Winograd-domain operands: V (forward planes), dM (transformed dY), dX (the padded dY planes of the
  // transposed-conv form of the input gradient); the 6-point forms only (F(2,3) planes feed the fp32-operand kernels)
  const bool wslots = wm != 2;
  const size_t slV = wslots ? reserve_slot() : 0, slD = wslots ? reserve_slot() : 0, slX = wslots ? reserve_slot() : 0;
  // pair-form planes (ops.h wino_input_transform): V feeds the forward GEMM and the weight gradient, dM the weight gradient and
  // the adjoint-form input gradient, dX (transposed-conv form of the input gradient) its one GEMM
  const bool wgrad_pairs = wslots && conv_wgrad_takes_pairs(wT, Cip, Cop);
  const bool pairV_ok = wslots && wino_fwd_takes_pairs(Cip, Cop) && (!y.has_grad || wgrad_pairs);
  const bool pairD_ok = wslots && wgrad_pairs && (!(wadj && x.has_grad && y.has_grad) || wino_fwd_takes_pairs(Cop, Cip));
  const bool pairX_ok = wslots && wino_fwd_takes_pairs(Cop, Cip);
  const size_t kV = wslots ? reserve_k() : 0, kD = wslots ? reserve_k() : 0, kX = wslots ? reserve_k() : 0;
  // dM = A dY A^T, shared by the weight gradient (side stream) and the adjoint-form input gradient
  float* keepdM = (wadj && y.has_grad && x.has_grad && share_dy()) ? static_cast<float*>(ctx.alloc((size_t)wP * wT * Cop * sizeof(float))) : nullptr;
  const size_t pcw_off = pcw ? reserve_dgp(pcw_bs * wP) : 0, uf_off = pcw ? 0 : reserve_dg(self, (size_t)wP * Cip * Cop);
  wsV_need = std::max(wsV_need, std::max((size_t)wP * wT * std::max(Cip, Cop), (size_t)wP * wT2 * Cop));
  wsM_need = std::max(wsM_need, std::max((size_t)wP * wT * std::max(Cip, Cop), (size_t)wP * wT2 * Cip));
  wsU_need = std::max(wsU_need, (size_t)wP * Cip * Cop);
  // amax slot of the output buffer (round 5): the 6-point output transform folds its output's amax -- VGG16's conv + ReLU layers
  // feed the next conv directly; everything else here is followed by a norm_act, which folds for its own output
  const bool y_folds = actf != ACT_NONE && actf != ACT_TANH && wm != 2;
  const size_t ySlot = note_writer(y.vbase, y_folds);
  const float* xbase = x.vbase;
  op.fwd = [=](Net& n) {
    n.need(self);
    float* V = keepV ? keepV : n.wsV;
    const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
    wino_input_transform(n.ctx.s, wm, wr, xv, 1, gf.pad_mode, wTh, wTw, V, wslots ? n.amax + slV : nullptr, xin, n.kscale + kV);
    conv_fwd(n.ctx.s, plane_gemm(V, n.wsM, wT, Cip, Cop, Co, wP, plane_scale(xin != nullptr, n.kscale + kV, wslots ? n.amax + slV : nullptr),
                                 {pcw ? nullptr : n.dg + uf_off, n.dgp + pcw_off, pcw, pcw_bs}));
    wino_output_transform(n.ctx.s, wm, wr, n.wsM, Cop, wTh, wTw, bi >= 0 ? A->w + A->params[bi].off : nullptr, actf, yv, Co, 0,
                          y_folds ? n.amax + ySlot : nullptr);
  };

  // ---- backward plan
  Var scratch;       // dR when an activation is fused into the epilogue
  if (y.has_grad && actf != ACT_NONE) scratch = alloc_var(yv.N, yv.H, yv.W, Cop, false);
  const bool want_dx = x.has_grad && y.has_grad;
  // the input gradient's filters: U flipped and transposed (transposed-conv form) or with the channel axes swapped (adjoint form)
  const int pcwt = (want_dx && wm != 2) ? wino_precut_tile(Cop, Cip) : 0;
  const size_t pcwt_bs = pcwt ? conv_precut_elems(Cop, Cip, pcwt) : 0;
  size_t pcwt_off = 0, ub_off = 0;
  if (want_dx) {
    if (pcwt) pcwt_off = reserve_dgp(pcwt_bs * wP);
    else ub_off = reserve_dg(self, (size_t)wP * Cop * Cip);
    op.grad_targets.push_back(x);
  }
  op.repack = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    const float* wmax = nullptr;       // both directions transform the same packed parameter: one amax pass
    if (pcw) wino_filter_transform_pc(n.ctx.s, wm, wr, wd.ws, 0, A->w + wd.off, pcw, n.dgp + pcw_off, pcw_bs, &wmax);
    else wino_filter_transform(n.ctx.s, wm, wr, wd.ws, 0, A->w + wd.off, n.dg + uf_off);
    if (want_dx) {
      if (pcwt) wino_filter_transform_pc(n.ctx.s, wm, wr, wd.ws, wadj ? 2 : 1, A->w + wd.off, pcwt, n.dgp + pcwt_off, pcwt_bs, &wmax);
      else wino_filter_transform(n.ctx.s, wm, wr, wd.ws, wadj ? 2 : 1, A->w + wd.off, n.dg + ub_off);
    }
  };
  const TView ygv = y.g, xgv = x.g, scr = scratch.v;
  const bool has_ygrad = y.has_grad;
  const size_t scrSlot = (y.has_grad && actf != ACT_NONE) ? note_writer(scratch.v.p, true) : 0;      // (dY's amax: as in conv_direct)
  const float* ygbase = y.gbase;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    TView dY = ygv;
    const float* dy_slot = nullptr;
    if (actf != ACT_NONE) { act_bwd(n.ctx.s, ygv, yv, scr, actf, 0, n.amax + scrSlot); dY = scr; dy_slot = n.amax + scrSlot; }
    else dy_slot = n.slot_if_complete(ygbase);
    const ParamDesc& wd = A->params[wi];
    const bool dx_now = want_dx && !(me.reads_net_input && !igrad);
    // adjoint-form layers: the weight gradient and the input gradient multiply by the same dM planes -- transformed once, on the
    // main stream, into the layer's own buffer (the side stream reads it while the main stream moves on)
    const bool shared = keepdM && wgrad && dx_now;
    const float* xin = pairV_ok ? n.slot_if_complete(xbase) : nullptr;
    const float* din = pairD_ok ? dy_slot : nullptr;            // amax of dY bounds its planes
    float* const slotV = wslots ? n.amax + slV : nullptr;
    float* const slotD = wslots ? n.amax + slD : nullptr;
    const PlaneScale dMs = plane_scale(din != nullptr, n.kscale + kD, slotD);
    const PlanePanel Ut{pcwt ? nullptr : n.dg + ub_off, n.dgp + pcwt_off, pcwt, pcwt_bs};
    if (shared) wino_dy_transform(n.ctx.s, wm, wr, dY, wTh, wTw, keepdM, slotD, din, n.kscale + kD);
    if (wgrad) {
      Stream& sw = n.wgrad_stream();          // dY is final: the weight-gradient work may run beside the dgrad chain
      // dU[t] = V[t]^T dM[t] (wP batched reductions over the tiles), then dW = G^T dU G
      float* V = keepV ? keepV : n.wsV;
      float* dM = shared ? keepdM : n.wgrad_planes(sw);
      if (!keepV) wino_input_transform(sw, wm, wr, xv, 1, gf.pad_mode, wTh, wTw, V, slotV, xin, n.kscale + kV);
      if (!shared) wino_dy_transform(sw, wm, wr, dY, wTh, wTw, dM, slotD, din, n.kscale + kD);
      conv_wgrad(sw, plane_wgrad(V, dM, n.wsU, wT, Cip, Cop, Co, wP, plane_scale(xin != nullptr, n.kscale + kV, slotV), dMs));
      wino_filter_grad(sw, wm, wr, wd.ws, n.wsU, A->g + wd.off);
      // (bias gradient on the main stream where no input gradient is formed: see conv_direct)
      if (bi >= 0) n.bias_grad_of((!dx_now && bias_on_main()) ? n.ctx.s : sw, dY, A->g + A->params[bi].off);
    }
    if (!dx_now) return;
    const int accf = me.acc.empty() ? 0 : me.acc[0];
    if (!wadj) {
      // input gradient = the transposed stride-1 conv over dY (flipped, channel-transposed filter)
      const float* xdin = pairX_ok ? dy_slot : nullptr;
      float* const slotX = wslots ? n.amax + slX : nullptr;
      wino_input_transform(n.ctx.s, wm, wr, dY, wpad2, PAD_ZERO, wTh2, wTw2, n.wsV, slotX, xdin, n.kscale + kX);
      conv_fwd(n.ctx.s, plane_gemm(n.wsV, n.wsM, wT2, Cop, Cip, Cip, wP, plane_scale(xdin != nullptr, n.kscale + kX, slotX), Ut));
      wino_output_transform(n.ctx.s, wm, wr, n.wsM, Cip, wTh2, wTw2, nullptr, ACT_NONE, xgv, Cip, accf);
      return;
    }
    // input gradient in the forward tiling: dM = A dY A^T, dV = dM U^T (U with the channel axes swapped), then the adjoint
    // of the input transform scatters the patches BT^T dV BT back through the forward gather (padding rule included)
    float* dMx = shared ? keepdM : n.wsV;
    if (!shared) wino_dy_transform(n.ctx.s, wm, wr, dY, wTh, wTw, dMx, slotD, din, n.kscale + kD);
    conv_fwd(n.ctx.s, plane_gemm(dMx, n.wsM, wT, Cop, Cip, Cip, wP, dMs, Ut));
    wino_input_adjoint(n.ctx.s, wm, wr, n.wsM, Cip, 1, gf.pad_mode, wTh, wTw, xgv, accf);
  };
}

// The direct kernels: the plain implicit GEMM, the folded tail conv, and the input gradient as a four-phase (k4 s2), stride-1
// or reflect-folded forward-type launch over dY
void Net::conv_direct(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const ConvKind kind = L.kind;
  const int Co = L.Co, Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi, actf = L.actf, dgrad_C = L.dgrad_C;
  ParamArena* A = &arena; Op* self = &op;
  const Gather gf = L.geo.fwd;
  const TView xv = x.v, yv = y.v;
  const WShape& ws = arena.params[wi].ws;
  // tail conv: run as 4 folded sub-pixel phases on the un-upsampled input (25 instead of 64
  // taps per 2x2 outputs; see ops.h tail_fold_weights).  The folded weights and the folded
  // weight-gradient scratch live next to the dgrad operands and follow arena.version.
  const bool folded = kind == CK_TAIL_UP;
  const size_t fe = folded ? tail_fold_offset(ws, 4) : 0;
  const size_t fold_off = folded ? reserve_dg(self, fe) : 0, dfold_off = folded ? reserve_dg(self, fe) : 0;
  // weight panel pre-cut for the ring kernel (ops.h conv_precut): plain forward convs multiply by the arena weights themselves
  const int Kf = gf.KH * gf.KW * Cip;
  const int pc_f = !folded ? conv_precut_tile(Cip, ws.Npad) : 0;
  const size_t pcf_off = pc_f ? reserve_dgp(conv_precut_elems(Kf, ws.Npad, pc_f)) : 0;
  // amax slot of the output buffer: a direct conv with a fused activation feeds the next GEMM without a normalisation in
  // between (UNetDown without InstanceNorm, PatchGAN model.0), so it folds its output's amax (in the ring kernel's epilogue, else
  // by a pass: ops.h ConvFwdArgs::y_amax); everything else here is followed by a norm_act, which folds for its own output
  const bool y_folds = !folded && actf != ACT_NONE && actf != ACT_TANH;
  const size_t ySlot = note_writer(y.vbase, y_folds);
  const float* xbase = x.vbase;
  // Conv + InstanceNorm fusion: a plain direct conv above the register-resident InstanceNorm's 1024 pixels offers the
  // statistics' partial sums of its raw output from its epilogue (taken up by Net::norm_act if one normalises this buffer)
  double* stat_partial = nullptr;
  std::shared_ptr<bool> stat_use;
  {
    const int HoWo = yv.H * yv.W;
    const bool stats_on = env_on(getenv("SWN_CONV_STATS"));       // (A/B: read when a model is built)
    const int chunk = (stats_on && pc_f == 128 && actf == ACT_NONE && HoWo > 1024 && yv.cs == yv.C && yv.p == y.vbase)
                          ? conv_fwd_stat_chunk(Cip, ws.Npad, HoWo, yv.N, Kf) : 0;
    if (chunk) {
      const int chunks = HoWo / chunk;
      stat_partial = static_cast<double*>(ctx.alloc((size_t)yv.N * chunks * yv.C * 2 * sizeof(double)));
      stat_use = std::make_shared<bool>(false);
      conv_stats[y.vbase] = StatLink{stat_partial, chunks, stat_use};
    }
  }
  op.fwd = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    ConvFwdArgs a;
    a.x = xv; a.g = gf; a.w = A->w + wd.off; a.Npad = wd.ws.Npad;
    a.x_amax = n.slot_if_complete(xbase);
    if (y_folds) a.y_amax = n.amax + ySlot;
    if (stat_use && *stat_use) a.stat_partial = stat_partial;
    if (pc_f) { n.need(self); a.wpc = n.dgp + pcf_off; a.wpc_bn = pc_f; }
    a.bias = bi >= 0 ? A->w + A->params[bi].off : nullptr;
    a.act = actf; a.y = yv; a.Cout = Co;
    if (!folded) { conv_fwd(n.ctx.s, a); return; }
    n.need(self);                            // folded weights are derived operands too
    a.x_amax = nullptr;
    a.g = Gather(); a.g.KH = a.g.KW = 3; a.g.stride = 1; a.g.pad_t = a.g.pad_l = 1; a.g.Ho = xv.H; a.g.Wo = xv.W;
    a.om.ymul = a.om.xmul = 2; a.tail4 = 1;
    a.w = n.dg + fold_off;
    conv_fwd(n.ctx.s, a);
  };

  // ---- backward plan
  Var scratch;       // dR when an activation is fused into the epilogue
  // tail conv: dR lives in a 32-channel buffer (pads stay zero) so that its input gradient -- a 5x5 stride-2 conv over dR with
  // K = 25 x Cop -- meets the ring kernel's 16-channel stages (K = 800 on the bf16-split ring kernel instead of K = 500 on the
  // register-staged f32-MFMA one)
  const int CopD = (folded && actf != ACT_NONE && Cop <= 32 && x.has_grad && conv_precut_tile(32, Cip) == 192) ? 32 : Cop;
  if (y.has_grad && actf != ACT_NONE) scratch = alloc_var(yv.N, yv.H, yv.W, CopD, false);
  Var dxpad;
  int dg_mode = 0;
  Gather gd;         // dgrad gather over dY
  int dHo = x.v.H, dWo = x.v.W;
  switch (kind) {
    case CK_K4S2: dg_mode = 0; break;
    case CK_K3S1_REFLECT:
      dg_mode = 1; gd.KH = gd.KW = 3; gd.stride = 1; gd.pad_t = gd.pad_l = 2; dHo = x.v.H + 2; dWo = x.v.W + 2; break;
    case CK_K3S1_ZERO: dg_mode = 1; gd.KH = gd.KW = 3; gd.stride = 1; gd.pad_t = gd.pad_l = 1; break;
    case CK_K4S1: dg_mode = 1; gd.KH = gd.KW = 4; gd.stride = 1; gd.pad_t = gd.pad_l = 2; break;
    case CK_K1S1: dg_mode = 1; gd.KH = gd.KW = 1; gd.stride = 1; gd.pad_t = gd.pad_l = 0; break;
    case CK_TAIL_UP: dg_mode = 3; gd.KH = gd.KW = 5; gd.stride = 2; gd.pad_t = gd.pad_l = 1; break;
  }
  gd.Ho = dHo; gd.Wo = dWo;
  const bool want_dx = x.has_grad && y.has_grad;
  // dgrad output channels = input buffer channels -- or, for a layer that reads a network input of which only the leading
  // channels are anyone's output (the generator's image inside the conditional discriminator's input), just those
  const bool narrow_dx = dgrad_C > 0 && dgrad_C % 4 == 0 && dgrad_C < Cip && (kind == CK_K4S2 || kind == CK_K3S1_ZERO);
  const int Ndg = narrow_dx ? dgrad_C : Cip;
  // K4S2: four phase panels of 2x2 taps; stride-1: one panel of KH x KW taps over dY (Cop channels)
  const int dpanels = kind == CK_K4S2 ? 4 : 1;
  const int dKp = (kind == CK_K4S2 ? 4 : gd.KH * gd.KW) * CopD;
  size_t dg_off = 0, pcd_off = 0;
  int pc_d = 0;
  if (want_dx) {
    dg_off = reserve_dg(self, dgrad_elems(ws, dg_mode, CopD, Ndg));
    if (kind == CK_K3S1_REFLECT) dxpad = alloc_var(x.v.N, dHo, dWo, Cip, false);
    op.grad_targets.push_back(narrow_dx ? x.slice(0, Ndg) : x);
    pc_d = conv_precut_tile(CopD, Ndg);
    if (pc_d) pcd_off = reserve_dgp(conv_precut_elems(dKp, Ndg, pc_d) * dpanels);
  }
  const size_t pcd_bs = pc_d ? conv_precut_elems(dKp, Ndg, pc_d) : 0;
  if (pc_f || want_dx || folded)
    op.repack = [=](Net& n) {
      const ParamDesc& wd = A->params[wi];
      // the forward operand first: the partial maxima its pre-cut takes are handed to the input-gradient operand's (ops.h
      // conv_precut amax_io), which runs right behind it
      const float* wmax = nullptr;
      if (pc_f) conv_precut(n.ctx.s, A->w + wd.off, Kf, wd.ws.Npad, pc_f, 1, 0, n.dgp + pcf_off, &wmax);
      if (want_dx) {
        repack_dgrad(n.ctx.s, wd.ws, dg_mode, CopD, Ndg, A->w + wd.off, n.dg + dg_off);
        // (the re-pack is a permutation of the parameter -- of its leading input channels if the gradient is narrow: the partial
        // maxima the forward operand's pre-cut just took, if it ran in front of us, bound it)
        if (pc_d) conv_precut(n.ctx.s, n.dg + dg_off, dKp, Ndg, pc_d, dpanels, (size_t)dKp * Ndg, n.dgp + pcd_off, &wmax);
      }
      if (folded) tail_fold_weights(n.ctx.s, wd.ws, A->w + wd.off, n.dg + fold_off);
    };
  const TView ygv = y.g, xgv = narrow_dx ? x.g.slice(0, Ndg) : x.g, scr = CopD != Cop ? scratch.v.slice(0, Cop) : scratch.v, scr_full = scratch.v, dxp = dxpad.v;
  const bool has_ygrad = y.has_grad;
  // dY as a GEMM operand: dR from act_bwd (which folds its amax into the scratch buffer's slot) or y.g itself, whose slot --
  // if it has one -- the norm_act behind this conv fills in its backward
  const size_t scrSlot = (y.has_grad && actf != ACT_NONE) ? note_writer(scratch.v.p, true) : 0;
  const float* ygbase = y.gbase;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    TView dY = ygv;
    const float* dy_slot = nullptr;
    if (actf != ACT_NONE) { act_bwd(n.ctx.s, ygv, yv, scr, actf, 0, n.amax + scrSlot); dY = scr; dy_slot = n.amax + scrSlot; }
    else dy_slot = n.slot_if_complete(ygbase);
    const ParamDesc& wd = A->params[wi];
    const bool dx_now = want_dx && !(me.reads_net_input && !igrad);
    if (wgrad) {
      Stream& sw = n.wgrad_stream();          // dY is final: the weight-gradient work may run beside the dgrad chain
      ConvWgradArgs wa;
      wa.x = xv; wa.g = gf; wa.dy = dY; wa.dw = A->g + wd.off; wa.Npad = wd.ws.Npad; wa.Cout = Co;
      wa.x_amax = n.slot_if_complete(xbase); wa.dy_amax = dy_slot;
      if (!folded) {
        conv_wgrad(sw, wa);
      } else {
        wa.x_amax = wa.dy_amax = nullptr;
        wa.g = Gather(); wa.g.KH = wa.g.KW = 3; wa.g.stride = 1; wa.g.pad_t = wa.g.pad_l = 1; wa.g.Ho = xv.H; wa.g.Wo = xv.W;
        wa.om.ymul = wa.om.xmul = 2; wa.tail4 = 1;
        wa.dw = n.dg + dfold_off;
        conv_wgrad(sw, wa);
        tail_unfold_wgrad(sw, wd.ws, n.dg + dfold_off, A->g + wd.off);
      }
      // bias gradient: beside the weight gradient on the second stream -- unless this layer forms no input gradient (the first layer of
      // a pass: PatchGAN's model.0 in backward_D, whose weight gradient is the step's exposed tail), where the main stream has nothing
      // else to do and the column sums run there, beside the weight gradient instead of behind it (round 6; same kernel, bit-identical)
      if (bi >= 0) n.bias_grad_of((!dx_now && bias_on_main()) ? n.ctx.s : sw, dY, A->g + A->params[bi].off);
    }
    if (!dx_now) return;
    const int accf = me.acc.empty() ? 0 : me.acc[0];
    ConvFwdArgs d;
    d.w = n.dg + dg_off; d.Npad = Ndg; d.Cout = Ndg;
    d.x_amax = dy_slot;
    if (pc_d) { d.wpc = n.dgp + pcd_off; d.wpc_bn = pc_d; d.wpc_bs = pcd_bs; }
    if (kind == CK_K4S2) {
      // four sub-pixel phases of the transposed conv (2x2 taps each) in one launch
      d.x = dY; d.g.KH = d.g.KW = 2; d.g.stride = 1; d.g.pad_t = 1; d.g.pad_l = 1;
      d.g.Ho = dY.H; d.g.Wo = dY.W;
      d.w_bs = (size_t)4 * Cop * Ndg;
      d.y = xgv; d.om.ymul = 2; d.om.xmul = 2; d.phases = 4; d.accumulate = accf;
      conv_fwd(n.ctx.s, d);
    } else if (kind == CK_K3S1_REFLECT) {
      d.x = dY; d.g = gd; d.y = dxp; d.accumulate = 0;
      conv_fwd(n.ctx.s, d);
      reflect_fold(n.ctx.s, dxp, xgv, accf);
    } else {
      d.x = CopD != Cop ? scr_full : dY; d.g = gd; d.y = xgv; d.accumulate = accf;
      conv_fwd(n.ctx.s, d);
    }
  };
}

// ---- ConvTranspose2d k4 s2 p1 (modules/layers.py:31, pix2pix_modules.py:226-246) ------
void Net::convT(const std::string& name, const Var& x, const Var& y, int Co, bool bias) {
  const WinoSwitches sw = wino_switches();
  if (y.v.H != x.v.H * 2 || y.v.W != x.v.W * 2) throw Error(1, "convT " + name + ": output view has the wrong size");
  const int Cip = x.v.C, Cop = round_up(Co, 4);
  if (y.v.C != Cop) throw Error(1, "convT " + name + ": output view must have round_up(Co,4) channels");
  const int wi = arena.add_weight(name + ".weight", WK_CONVT, Co, Cip, 4, 4, Cip, nullptr);
  const int bi = bias ? arena.add_bias(name + ".bias", Co) : -1;
  auto op = std::make_unique<Op>();
  op->label = name;
  op->param_off = arena.params[wi].off;
  note_writer(y.vbase, false);        // (raw output: always followed by an InstanceNorm, never a GEMM operand itself)
  const ConvLayer L{name, x, y, CK_K4S2, Cip, Co, Cip, Cop, wi, bi, ACT_NONE, ConvGeom(), false, 0};
  // enough channels: strided Winograd F(4x4,2x2) -- the transposed conv is the ADJOINT of a k4 s2 conv fine -> coarse, so its
  // forward is the coarse -> fine pipeline (dM = A x A^T, dV = dM U^T, adjoint polyphase transform) and its input gradient the
  // fine -> coarse one
  if (s2_wino && s2_wino_wanted(sw, Cop, Cip, x.v.H, x.v.W) && Co % 4 == 0) convT_wino_s2(L, *op);
  else convT_direct(L, *op);
  ops.push_back(std::move(op));
}

void Net::convT_wino_s2(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const int Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi;
  ParamArena* A = &arena; Op* self = &op;
  const TView xv = x.v, yv = y.v, ygv = y.g, xgv = x.g;
  const float* xbase = x.vbase; const float* ygbase = y.gbase;
  const int sP = 25, sTh = ceil_div(x.v.H, 4), sTw = ceil_div(x.v.W, 4), CV = 4 * Cop;
  const size_t sT = (size_t)x.v.N * sTh * sTw;
  const bool want_dx = x.has_grad && y.has_grad;
  const size_t ut_off = reserve_dg(self, (size_t)sP * Cip * CV);                      // U^T[25][Cip][4 Cop]   (forward)
  const size_t uf_off = want_dx ? reserve_dg(self, (size_t)sP * CV * Cip) : 0;        // U  [25][4 Cop][Cip]   (input gradient)
  float* keepM = (keep_wino_inputs && y.has_grad) ? static_cast<float*>(ctx.alloc(sP * sT * Cip * sizeof(float))) : nullptr;
  wsV_need = std::max(wsV_need, sP * sT * (size_t)std::max(CV, Cip));
  wsM_need = std::max(wsM_need, sP * sT * (size_t)std::max(CV, Cip));
  wsU_need = std::max(wsU_need, (size_t)sP * CV * Cip);
  const int pct = conv_precut_tile(Cip, CV), pcf = want_dx ? conv_precut_tile(CV, Cip) : 0;
  const size_t pct_bs = pct ? conv_precut_elems(Cip, CV, pct) : 0, pcf_bs = pcf ? conv_precut_elems(CV, Cip, pcf) : 0;
  const size_t pct_off = pct ? reserve_dgp(pct_bs * sP) : 0, pcf_off = pcf ? reserve_dgp(pcf_bs * sP) : 0;
  const size_t slM = reserve_slot(), slV = reserve_slot();     // amax of dM (planes of the coarse input) and of V (planes of dY, fine)
  const bool wg_pairs = conv_wgrad_takes_pairs(sT, CV, Cip);
  const bool pairM_ok = conv_fwd_takes_pairs(Cip, CV) && (!y.has_grad || wg_pairs);
  const bool pairV_ok = wg_pairs && (!(x.has_grad && y.has_grad) || conv_fwd_takes_pairs(CV, Cip));
  const size_t kM = reserve_k(), kVg = reserve_k();
  // V = polyphase transform of dY serves the weight gradient (side stream) and the input gradient (main stream): one buffer per layer
  float* keepVg = (y.has_grad && want_dx && share_dy()) ? static_cast<float*>(ctx.alloc(sP * sT * CV * sizeof(float))) : nullptr;
  op.repack = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    wino_s2_filter_transform(n.ctx.s, wd.ws, 1, A->w + wd.off, n.dg + ut_off);
    const float* wmax = nullptr;
    if (pct) conv_precut(n.ctx.s, n.dg + ut_off, Cip, CV, pct, sP, (size_t)Cip * CV, n.dgp + pct_off, &wmax);
    if (want_dx) {
      wino_s2_filter_transform(n.ctx.s, wd.ws, 0, A->w + wd.off, n.dg + uf_off);
      if (pcf) conv_precut(n.ctx.s, n.dg + uf_off, CV, Cip, pcf, sP, (size_t)CV * Cip, n.dgp + pcf_off, &wmax);
    }
  };
  op.fwd = [=](Net& n) {
    n.need(self);
    float* dM = keepM ? keepM : n.wsV;
    const float* xin = pairM_ok ? n.slot_if_complete(xbase) : nullptr;
    wino_dy_transform(n.ctx.s, 4, 2, xv, sTh, sTw, dM, n.amax + slM, xin, n.kscale + kM);
    conv_fwd(n.ctx.s, plane_gemm(dM, n.wsM, sT, Cip, CV, CV, sP, plane_scale(xin != nullptr, n.kscale + kM, n.amax + slM),
                                 {n.dg + ut_off, n.dgp + pct_off, pct, pct_bs}));
    wino_s2_input_adjoint(n.ctx.s, n.wsM, Cop, sTh, sTw, yv, bi >= 0 ? A->w + A->params[bi].off : nullptr, 0);
  };
  if (want_dx) op.grad_targets.push_back(x);
  const bool has_ygrad = y.has_grad;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    const ParamDesc& wd = A->params[wi];
    const bool dx_now = want_dx && !(me.reads_net_input && !igrad);
    const bool shared = keepVg && wgrad && dx_now;
    const float* xin = pairM_ok ? n.slot_if_complete(xbase) : nullptr;
    const float* din = pairV_ok ? n.slot_if_complete(ygbase) : nullptr;
    const PlaneScale Vs = plane_scale(din != nullptr, n.kscale + kVg, n.amax + slV);
    if (shared) wino_s2_input_transform(n.ctx.s, ygv, sTh, sTw, keepVg, n.amax + slV, din, n.kscale + kVg);
    if (wgrad) {
      // dU[25][4 Cop][Cip] = V(dY fine)^T dM(x coarse)
      Stream& sw = n.wgrad_stream();
      float* V = shared ? keepVg : n.wgrad_planes(sw);
      float* dM = keepM ? keepM : n.wsV;
      if (!shared) wino_s2_input_transform(sw, ygv, sTh, sTw, V, n.amax + slV, din, n.kscale + kVg);
      if (!keepM) wino_dy_transform(sw, 4, 2, xv, sTh, sTw, dM, n.amax + slM, xin, n.kscale + kM);
      conv_wgrad(sw, plane_wgrad(V, dM, n.wsU, sT, CV, Cip, Cip, sP, Vs, plane_scale(xin != nullptr, n.kscale + kM, n.amax + slM)));
      wino_s2_filter_grad(sw, wd.ws, n.wsU, A->g + wd.off);
      if (bi >= 0) n.bias_grad_of(sw, ygv, A->g + A->params[bi].off);
    }
    if (!dx_now) return;
    float* Vx = shared ? keepVg : n.wsV;
    if (!shared) wino_s2_input_transform(n.ctx.s, ygv, sTh, sTw, Vx, n.amax + slV, din, n.kscale + kVg);
    conv_fwd(n.ctx.s, plane_gemm(Vx, n.wsM, sT, CV, Cip, Cip, sP, Vs, {n.dg + uf_off, n.dgp + pcf_off, pcf, pcf_bs}));
    wino_output_transform(n.ctx.s, 4, 2, n.wsM, Cip, sTh, sTw, nullptr, ACT_NONE, xgv, Cip, me.acc.empty() ? 0 : me.acc[0]);
  };
}

void Net::convT_direct(const ConvLayer& L, Op& op) {
  const Var &x = L.x, &y = L.y;
  const int Co = L.Co, Cip = L.Cip, Cop = L.Cop, wi = L.wi, bi = L.bi;
  ParamArena* A = &arena; Op* self = &op;
  const TView xv = x.v, yv = y.v, ygv = y.g, xgv = x.g;
  const float* xbase = x.vbase; const float* ygbase = y.gbase;
  const size_t phase_elems = (size_t)4 * Cip * round_up(Co, 4);
  // pre-cut panels for the ring kernel: the four forward phase panels (arena layout) and the k4 s2 input-gradient operand
  const int pc_f = conv_precut_tile(Cip, Cop);
  const size_t pcf_bs = pc_f ? conv_precut_elems(4 * Cip, Cop, pc_f) : 0;
  const size_t pcf_off = pc_f ? reserve_dgp(pcf_bs * 4) : 0;
  op.fwd = [=](Net& n) {
    const ParamDesc& wd = A->params[wi];
    ConvFwdArgs f;                          // 4 sub-pixel phases (2x2 taps each), one launch
    if (pc_f) { n.need(self); f.wpc = n.dgp + pcf_off; f.wpc_bn = pc_f; f.wpc_bs = pcf_bs; }
    f.x = xv; f.g.KH = f.g.KW = 2; f.g.stride = 1; f.g.pad_t = 1; f.g.pad_l = 1; f.g.Ho = xv.H; f.g.Wo = xv.W;
    f.w = A->w + wd.off; f.w_bs = phase_elems; f.Npad = wd.ws.Npad;
    f.x_amax = n.slot_if_complete(xbase);
    f.bias = bi >= 0 ? A->w + A->params[bi].off : nullptr;
    f.y = yv; f.om.ymul = 2; f.om.xmul = 2; f.phases = 4; f.Cout = Co;
    conv_fwd(n.ctx.s, f);
  };
  const bool want_dx = x.has_grad && y.has_grad;
  size_t dg_off = 0, pcd_off = 0;
  const int pc_d = want_dx ? conv_precut_tile(Cop, Cip) : 0;
  if (want_dx) {
    dg_off = reserve_dg(self, dgrad_elems(arena.params[wi].ws, 2, Cop, Cip));
    if (pc_d) pcd_off = reserve_dgp(conv_precut_elems(16 * Cop, Cip, pc_d));
    op.grad_targets.push_back(x);
  }
  if (want_dx || pc_f)
    op.repack = [=](Net& n) {
      const ParamDesc& wd = A->params[wi];
      const float* wmax = nullptr;       // the k4 s2 re-pack permutes the four phase panels: one amax pass
      if (pc_f) conv_precut(n.ctx.s, A->w + wd.off, 4 * Cip, Cop, pc_f, 4, phase_elems, n.dgp + pcf_off, &wmax);
      if (want_dx) {
        repack_dgrad(n.ctx.s, wd.ws, 2, Cop, Cip, A->w + wd.off, n.dg + dg_off);
        if (pc_d) conv_precut(n.ctx.s, n.dg + dg_off, 16 * Cop, Cip, pc_d, 1, 0, n.dgp + pcd_off, &wmax);
      }
    };
  const bool has_ygrad = y.has_grad;
  op.bwd = [=](Net& n, Op& me, bool wgrad, bool igrad) {
    if (!has_ygrad) return;
    const ParamDesc& wd = A->params[wi];
    if (wgrad) {
      ConvWgradArgs wa;
      wa.x = xv; wa.g.KH = wa.g.KW = 2; wa.g.stride = 1; wa.g.pad_t = 1; wa.g.pad_l = 1;
      wa.g.Ho = xv.H; wa.g.Wo = xv.W;
      wa.dy = ygv; wa.om.ymul = 2; wa.om.xmul = 2; wa.phases = 4;
      wa.dw = A->g + wd.off; wa.dw_bs = phase_elems; wa.Npad = wd.ws.Npad; wa.Cout = Co;
      wa.x_amax = n.slot_if_complete(xbase); wa.dy_amax = n.slot_if_complete(ygbase);
      Stream& sw = n.wgrad_stream();
      conv_wgrad(sw, wa);
      if (bi >= 0) n.bias_grad_of(sw, ygv, A->g + A->params[bi].off);
    }
    if (!want_dx || (me.reads_net_input && !igrad)) return;
    ConvFwdArgs d;
    d.x = ygv; d.g.KH = d.g.KW = 4; d.g.stride = 2; d.g.pad_t = d.g.pad_l = 1; d.g.Ho = xv.H; d.g.Wo = xv.W;
    d.w = n.dg + dg_off; d.Npad = Cip; d.Cout = Cip; d.y = xgv; d.accumulate = me.acc.empty() ? 0 : me.acc[0];
    d.x_amax = n.slot_if_complete(ygbase);
    if (pc_d) { d.wpc = n.dgp + pcd_off; d.wpc_bn = pc_d; }
    conv_fwd(n.ctx.s, d);
  };
}

// ---- [InstanceNorm] -> act -> [dropout] (+ residual) -----------------------------------
void Net::norm_act(const Var& raw, const Var& y, bool norm, int actf, float drop_p, const Var* residual) {
  auto op = std::make_unique<Op>();
  op->label = "norm_act";
  float* stats = norm ? static_cast<float*>(ctx.alloc((size_t)raw.v.N * raw.v.C * 2 * sizeof(float))) : nullptr;
  last_stats = stats;
  const uint64_t salt = ops.size() + 1;
  if (drop_p > 0.f) drop_sites.push_back({salt, raw.v.N, raw.v.H, raw.v.W, raw.v.C, drop_p});
  if (residual && actf != ACT_NONE) throw Error(1, "norm_act: an activation in front of a residual add is not supported");
  note_act(actf, y.v);        // a dropped element reads 0: its gradient is 0 whichever side the pattern records
  const TView rv = raw.v, rg = raw.g, yv = y.v, yg = y.g;
  const size_t ySlot = note_writer(y.vbase, true);
  const size_t gSlot = (y.has_grad && raw.has_grad) ? note_writer(raw.gbase, true) : 0;
  const bool has_res = residual != nullptr;
  const Var res = has_res ? *residual : Var();
  const double* partial_in = nullptr;
  int partial_chunks = 0;
  if (norm && raw.v.H * raw.v.W > 1024 && raw.v.p == raw.vbase) {
    auto it = conv_stats.find(raw.vbase);
    if (it != conv_stats.end()) { *it->second.use = true; partial_in = it->second.partial; partial_chunks = it->second.chunks; }
  }
  op->fwd = [=](Net& n) {
    NormActArgs a;
    a.x = rv; a.y = yv; a.stats = stats; a.norm = norm; a.act = actf;
    a.partial_in = partial_in; a.partial_chunks = partial_chunks;
    a.drop_p = n.training ? drop_p : 0.f; a.seed = Net::drop_seed(n.seed, salt);
    a.seed_base = n.seed_dev; a.salt = salt;
    a.residual = has_res ? &res.v : nullptr;
    a.amax_out = n.amax + ySlot;
    norm_act_fwd(n.ctx.s, a);
  };
  if (has_res && res.has_grad && y.has_grad) op->grad_targets.push_back(res);
  const bool do_bwd = y.has_grad && raw.has_grad;
  double* colsum = nullptr;
  if (do_bwd && norm && norm_act_bwd_emits_colsum(raw.v.H * raw.v.W, raw.v.C) && raw.g.cs == raw.g.C) {
    colsum = static_cast<double*>(ctx.alloc((size_t)raw.v.N * raw.v.C * sizeof(double)));
    colsums[raw.g.p] = {colsum, raw.v.N};
  }
  op->bwd = [=](Net& n, Op& me, bool, bool) {
    if (!do_bwd) return;
    if (has_res && res.has_grad) axpy(n.ctx.s, yg, res.g, 1.f, me.acc.empty() ? 0 : me.acc[0]);
    NormActBwdArgs b;
    b.dy = yg; b.x = rv; b.stats = stats; b.dx = rg; b.norm = norm; b.act = actf; b.colsum = colsum;
    b.drop_p = n.training ? drop_p : 0.f; b.seed = Net::drop_seed(n.seed, salt);
    b.seed_base = n.seed_dev; b.salt = salt;
    b.amax_out = n.amax + gSlot;
    norm_act_bwd(n.ctx.s, b);
  };
  ops.push_back(std::move(op));
}

// ---- BatchNorm2d -> act (batch_norm.hip) -------------------------------------------------
void Net::batch_norm_act(const std::string& name, const Var& raw, const Var& y, int actf, int groups, const BNBuffers& run,
                         float drop_p) {
  auto op = std::make_unique<Op>();
  op->label = "batch_norm_act";
  const int C = raw.v.C;
  const uint64_t salt = ops.size() + 1;
  if (drop_p > 0.f) drop_sites.push_back({salt, raw.v.N, raw.v.H, raw.v.W, raw.v.C, drop_p});
  const size_t goff = arena.params[arena.add_bias(name + ".weight", C)].off;
  const size_t boff = arena.params[arena.add_bias(name + ".bias", C)].off;
  op->param_off = goff;
  float* stats = static_cast<float*>(ctx.alloc((size_t)groups * C * 2 * sizeof(float)));
  float* fold = static_cast<float*>(ctx.alloc((size_t)groups * C * 2 * sizeof(float)));
  last_stats = stats;
  note_act(actf, y.v);
  const TView rv = raw.v, rg = raw.g, yv = y.v, yg = y.g;
  const size_t ySlot = note_writer(y.vbase, true);
  const bool do_bwd = y.has_grad && raw.has_grad;
  const size_t gSlot = do_bwd ? note_writer(raw.gbase, true) : 0;
  const double* partial_in = nullptr;
  int partial_chunks = 0;
  if (raw.v.H * raw.v.W > 1024 && raw.v.p == raw.vbase) {        // the producing conv's epilogue offers the partial sums (see norm_act)
    auto it = conv_stats.find(raw.vbase);
    if (it != conv_stats.end()) { *it->second.use = true; partial_in = it->second.partial; partial_chunks = it->second.chunks; }
  }
  op->fwd = [=](Net& n) {
    BatchNormArgs a;
    a.x = rv; a.y = yv; a.gamma = n.arena.w + goff; a.beta = n.arena.w + boff;
    a.running_mean = run.mean; a.running_var = run.var; a.num_batches_tracked = run.count;
    a.stats = stats; a.fold = fold; a.groups = groups; a.act = actf; a.training = n.bn_training ? 1 : 0;
    a.amax_out = n.amax + ySlot;
    if (n.bn_training) { a.partial_in = partial_in; a.partial_chunks = partial_chunks; }
    if (drop_p > 0.f && n.training && n.bn_training) {
      a.drop_p = drop_p; a.seed = Net::drop_seed(n.seed, salt); a.seed_base = n.seed_dev; a.salt = salt;
    }
    batch_norm_fwd(n.ctx.s, a);
  };
  op->bwd = [=](Net& n, Op&, bool wgrad, bool) {
    if (!do_bwd) return;
    if (!n.bn_training) throw Error(1, "batch_norm_act: backward through the eval-mode forward is not supported");
    BatchNormBwdArgs b;
    b.dy = yg; b.x = rv; b.stats = stats; b.fold = fold; b.dx = rg; b.groups = groups; b.act = actf;
    if (wgrad) { b.dgamma = n.arena.g + goff; b.dbeta = n.arena.g + boff; }
    if (drop_p > 0.f && n.training) {
      b.drop_p = drop_p; b.seed = Net::drop_seed(n.seed, salt); b.seed_base = n.seed_dev; b.salt = salt;
    }
    b.amax_out = n.amax + gSlot;
    batch_norm_bwd(n.ctx.s, b);
  };
  ops.push_back(std::move(op));
}

void Net::act(const Var& x, const Var& y, int actf) {
  auto op = std::make_unique<Op>();
  op->label = "act";
  const size_t ySlot = note_writer(y.vbase, true);        // (round 5: the element-wise kernel folds its output's amax like every other producer)
  note_act(actf, y.v);
  const TView xv = x.v, yv = y.v, xg = x.g, yg = y.g;
  op->fwd = [=](Net& n) { act_fwd(n.ctx.s, xv, yv, actf, n.amax + ySlot); };
  const bool do_bwd = x.has_grad && y.has_grad;
  if (do_bwd) op->grad_targets.push_back(x);
  op->bwd = [=](Net& n, Op& me, bool, bool) {
    if (do_bwd) act_bwd(n.ctx.s, yg, yv, xg, actf, me.acc.empty() ? 0 : me.acc[0]);
  };
  ops.push_back(std::move(op));
}

void Net::affine(const Var& x, const Var& y, float alpha, float shift) {
  auto op = std::make_unique<Op>();
  op->label = "affine";
  note_writer(y.vbase, false);        // (not a folding writer: forward_from() may skip this op -- the VGG slices are entered behind it with
                                      // a buffer the caller filled -- so its consumer takes the amax itself)
  const TView xv = x.v, yv = y.v, xg = x.g, yg = y.g;
  op->fwd = [=](Net& n) { axpy(n.ctx.s, xv, yv, alpha, 0, shift); };
  const bool do_bwd = x.has_grad && y.has_grad;
  if (do_bwd) op->grad_targets.push_back(x);
  op->bwd = [=](Net& n, Op& me, bool, bool) {
    if (do_bwd) axpy(n.ctx.s, yg, xg, alpha, me.acc.empty() ? 0 : me.acc[0], 0.f);
  };
  ops.push_back(std::move(op));
}

void Net::upsample(const Var& x, const Var& y, int f) {
  auto op = std::make_unique<Op>();
  op->label = "upsample";
  const size_t ySlot = note_writer(y.vbase, true);
  const TView xv = x.v, yv = y.v, xg = x.g, yg = y.g;
  op->fwd = [=](Net& n) { upsample_nearest_fwd(n.ctx.s, xv, yv, f, n.amax + ySlot); };
  const bool do_bwd = x.has_grad && y.has_grad;
  if (do_bwd) op->grad_targets.push_back(x);
  op->bwd = [=](Net& n, Op& me, bool, bool) {
    if (do_bwd) upsample_nearest_bwd(n.ctx.s, yg, xg, f, me.acc.empty() ? 0 : me.acc[0]);
  };
  ops.push_back(std::move(op));
}

void Net::maxpool(const Var& x, const Var& y) {
  auto op = std::make_unique<Op>();
  op->label = "maxpool";
  const size_t ySlot = note_writer(y.vbase, true);
  act_sites.push_back({2, y.v, x.v});
  const TView xv = x.v, yv = y.v, xg = x.g, yg = y.g;
  op->fwd = [=](Net& n) { maxpool2_fwd(n.ctx.s, xv, yv, n.amax + ySlot); };
  const bool do_bwd = x.has_grad && y.has_grad;
  if (do_bwd) op->grad_targets.push_back(x);
  op->bwd = [=](Net& n, Op& me, bool, bool) {
    if (!do_bwd) return;
    maxpool2_bwd(n.ctx.s, yg, xv, yv, xg, me.acc.empty() ? 0 : me.acc[0]);
  };
  ops.push_back(std::move(op));
}

void Net::custom(const std::string& label, std::function<void(Net&)> fwd,
                 std::function<void(Net&, const std::vector<int>& acc)> bwd, const std::vector<Var>& grad_targets) {
  auto op = std::make_unique<Op>();
  op->label = label;
  op->fwd = fwd ? fwd : [](Net&) {};
  op->grad_targets = grad_targets;
  op->bwd = [bwd](Net& n, Op& me, bool, bool) { if (bwd) bwd(n, me.acc); };
  ops.push_back(std::move(op));
}

// ---- accumulate planner -----------------------------------------------------------------
// Walk the tape backwards (the order backward() executes) and decide, per gradient write,
// whether it is the first producer of that (buffer, channel range) -> overwrite, or a later
// one -> accumulate.  A write that covers a partly-initialised range is a builder bug.
void Net::finalize(const std::vector<Var>& pre) {
  std::map<float*, std::vector<char>> seen;
  auto range = [&](const Var& v, int& c0, int& c1) -> std::vector<char>& {
    std::vector<char>& s = seen[v.gbase];
    if (s.empty()) s.assign(v.g.cs, 0);
    c0 = (int)((v.g.p - v.gbase) % v.g.cs);
    c1 = c0 + v.g.C;
    return s;
  };
  for (const Var& v : pre) {
    if (!v.has_grad) continue;
    int c0, c1;
    auto& s = range(v, c0, c1);
    for (int c = c0; c < c1; ++c) s[c] = 1;
  }
  for (int i = (int)ops.size() - 1; i >= 0; --i) {
    Op& op = *ops[i];
    op.acc.assign(op.grad_targets.size(), 0);
    for (size_t t = 0; t < op.grad_targets.size(); ++t) {
      const Var& v = op.grad_targets[t];
      int c0, c1;
      auto& s = range(v, c0, c1);
      int nset = 0;
      for (int c = c0; c < c1; ++c) nset += s[c];
      if (nset != 0 && nset != c1 - c0)
        throw Error(1, "accumulate planner: op '" + op.label + "' writes a partially initialised gradient range");
      op.acc[t] = nset ? 1 : 0;
      for (int c = c0; c < c1; ++c) s[c] = 1;
    }
  }
  dg = dg_n ? static_cast<float*>(ctx.alloc(dg_n * sizeof(float))) : nullptr;
  dgp = dgp_n ? static_cast<uint16_t*>(ctx.alloc(dgp_n * sizeof(uint16_t))) : nullptr;
  amax = amax_n ? static_cast<float*>(ctx.alloc(amax_n * sizeof(float))) : nullptr;
  kscale = kscale_n ? static_cast<int*>(ctx.alloc((kscale_n + 4) * sizeof(int))) : nullptr;
  if (wsM_need && ctx.has_side && keep_wino_inputs) wsM2 = static_cast<float*>(ctx.alloc(wsM_need * sizeof(float)));
  if (wsV_need) wsV = static_cast<float*>(ctx.alloc(wsV_need * sizeof(float)));
  if (wsM_need) wsM = static_cast<float*>(ctx.alloc(wsM_need * sizeof(float)));
  if (wsU_need) wsU = static_cast<float*>(ctx.alloc(wsU_need * sizeof(float)));
  finalized_ = true;
}

bool Net::share_dy() const { return keep_wino_inputs && ctx.has_side; }
void Net::forward() {
  if (!finalized_) throw Error(1, "Net::forward before finalize");
  if (amax) dev_memset(ctx.s, amax, 0, amax_n * sizeof(float));       // every slot: the step's producers fold into zeros
  prefetch_dgrad();
  for (auto& op : ops) { if (route_on()) route_label(op->label.c_str(), 'f'); op->fwd(*this); }
  prefetch_finish();
}
void Net::forward_from(int op_begin) {
  if (!finalized_) throw Error(1, "Net::forward before finalize");
  // every folding writer must lie at or behind op_begin (the frozen VGG16 slices are entered at op 1, behind a non-folding affine): a
  // skipped one would leave its buffer's slot at zero while consumers trust it as complete
  for (size_t w : fold_writer_ops)
    if (w < (size_t)op_begin) throw Error(1, "Net::forward_from(" + std::to_string(op_begin) + ") skips op " + std::to_string(w) +
                                             ", a folding writer of an amax slot");
  if (amax) dev_memset(ctx.s, amax, 0, amax_n * sizeof(float));
  prefetch_dgrad();
  for (size_t i = (size_t)op_begin; i < ops.size(); ++i) { if (route_on()) route_label(ops[i]->label.c_str(), 'f'); ops[i]->fwd(*this); }
  prefetch_finish();
}
// The operand refresh on the second stream, issued PIECEWISE (round 6).  Issuing all of it at the top of the pass -- ~130 launches and
// ~60 event records on the second stream in front of the pass's first kernel -- kept the main queue idle for 2.2 ms of every step: the
// runtime lets the host run only a bounded number of commands ahead of a queue, so the host sat inside that loop until the GPU had
// worked the batch down to its last dozen launches, and only then got to enqueue the forward pass (rocprofv3 --kernel-trace of bench.py,
// of bench.py on a stream of its own and of tools/native_ab alike: profiles/refresh_issue_order_r06.txt; tools/fork_probe.hip shows the
// events themselves release with single-kernel granularity when the host is ahead).  Now the pass starts with the operands of its first
// SWN_PREFETCH_AHEAD layers in flight and every layer, once its own operands are waited for, issues those of the layer that many places
// further down: both queues are fed in the order the GPU consumes them.  SWN_PREFETCH=3: everything at the top (the old order, for the
// A/B); 0: in order on the main stream.
int Net::prefetch_mode() {
  static const int mode = env_int(getenv("SWN_PREFETCH"), 1);
  return mode;
}
static size_t prefetch_ahead() {
  static const int n = std::max(1, env_int(getenv("SWN_PREFETCH_AHEAD"), 4));
  return (size_t)n;
}
void Net::prefetch_dgrad() {
  const int mode = prefetch_mode();
  if (mode == 0 || !ctx.use_side() || dg_version == arena.version || refresh_open_) return;
  if (repack_ops_.empty())
    for (size_t i = 0; i < ops.size(); ++i)
      if (ops[i]->repack) { ops[i]->repack_index = (int)repack_ops_.size(); repack_ops_.push_back(i); }
  if (repack_ops_.empty()) return;
  ctx.fork_side();                 // after the optimizer step that produced the weights and after every
                                   // main-stream reader of the previous operands
  refresh_open_ = true; refresh_pending = true; repack_next_ = 0;
  dg_version = arena.version;
  prefetch_issue(mode == 3 ? repack_ops_.size() : prefetch_ahead());
}
void Net::prefetch_issue(size_t upto) {
  upto = std::min(upto, repack_ops_.size());
  if (!refresh_open_ || repack_next_ >= upto) return;
  const std::string label_was = g_route_label; const char phase_was = g_route_phase;      // (called from inside a layer's forward)
  struct Relabel { const std::string& l; char p; ~Relabel() { g_route_label = l; g_route_phase = p; } } relabel{label_was, phase_was};
  std::swap(ctx.s, ctx.side);      // the re-pack launchers use ctx.s
  try {
    for (; repack_next_ < upto; ++repack_next_) {
      Op* op = ops[repack_ops_[repack_next_]].get();
      if (route_on()) route_label(op->label.c_str(), 'r');
      op->repack(*this);
      if (!op->ready) op->ready = event_create();
      event_record(op->ready, ctx.s);        // (ctx.s is the side stream here)
      op->ready_pending = true;
    }
  } catch (...) { std::swap(ctx.s, ctx.side); throw; }
  std::swap(ctx.s, ctx.side);
  if (repack_next_ == repack_ops_.size()) {
    if (!refresh_event) refresh_event = event_create();
    event_record(refresh_event, ctx.side);
    refresh_open_ = false;
  }
}
void Net::prefetch_finish() { if (refresh_open_) prefetch_issue(repack_ops_.size()); }
void Net::need(Op* op) {
  if (refresh_open_ && op->repack_index >= 0) prefetch_issue((size_t)op->repack_index + 1);      // (its own: normally issued layers ago)
  if (refresh_pending && op->ready_pending) {
    stream_wait_event(ctx.s, op->ready);
    op->ready_pending = false;
    if (refresh_open_) prefetch_issue((size_t)op->repack_index + 1 + prefetch_ahead());
    return;
  }
  if (!refresh_pending) refresh_dgrad();
}
void Net::refresh_dgrad() {
  if (refresh_pending) {
    prefetch_finish();
    stream_wait_event(ctx.s, refresh_event);
    refresh_pending = false;
    for (auto& op : ops) op->ready_pending = false;
  }
  if (dg_version == arena.version) return;
  for (auto& op : ops)
    if (op->repack) { if (route_on()) route_label(op->label.c_str(), 'r'); op->repack(*this); }
  dg_version = arena.version;
}
void Net::backward(bool wgrad, bool igrad) { backward_range(wgrad, igrad, 0, (int)ops.size()); }
void Net::backward_range(bool wgrad, bool igrad, int op_begin, int op_end, bool join) {
  for (int i = op_end - 1; i >= op_begin; --i) { if (route_on()) route_label(ops[i]->label.c_str(), 'b'); ops[i]->bwd(*this, *ops[i], wgrad, igrad); }
  if (join) ctx.join_side();      // weight gradients of the range are final for whatever the main stream does next
}
int Net::split_point(double frac, size_t* arena_off) const {
  const size_t want = (size_t)(frac * (double)arena.n);
  for (size_t i = 0; i < ops.size(); ++i)
    if (ops[i]->param_off != (size_t)-1 && ops[i]->param_off >= want) {
      if (arena_off) *arena_off = ops[i]->param_off;
      return (int)i;
    }
  if (arena_off) *arena_off = arena.n;
  return (int)ops.size();
}

// Bucket boundaries (fractions of the generator's gradient arena, high to low = backward order).
// WarpModule: [.70,1] = decoder + resblock convs 5-7, [.41,.70) = resblock convs 1-4, [.04,.41) = cloth_down5/6,
// cloth_up1/2, resblock conv 0, [0,.04) = body_down1-4 + cloth_down1-4.  Sized on the measured back-propagation time of the
// buckets (bench.py `dp_buckets`, 1 x MI355X, profiles/README.md): a bucket's exchange runs under the NEXT bucket's backward
// pass, so what matters is (a) every bucket but the last is followed by more backward time than its transfer takes at the
// ~170 GB/s algorithmic all-reduce rate of 8 GPUs over xGMI, and (b) the last bucket -- whose exchange and AdamW are exposed --
// is as small as (a) allows for the bucket before it: 22 MB (0.13 ms) instead of the 55 MB of round 2, with 2.5 ms of
// encoder back-propagation above the 240 MB transfer (1.4 ms) of the third bucket.  SWAPNET_GRAD_CUTS="f1,f2,..." overrides
// (descending fractions of the arena; read once).
static std::vector<double> grad_cuts() {
  static std::vector<double> cuts = [] {
    std::vector<double> c = {0.70, 0.41, 0.04};
    if (const char* e = getenv("SWAPNET_GRAD_CUTS")) {
      std::vector<double> u;
      for (const char* p = e; *p;) {
        char* end = nullptr;
        const double v = strtod(p, &end);
        if (end == p) break;
        u.push_back(v);
        p = *end == ',' ? end + 1 : end;
      }
      bool ok = !u.empty() && u.size() <= 15;
      for (size_t i = 0; i < u.size(); ++i) ok = ok && u[i] > 0.0 && u[i] < 1.0 && (i == 0 || u[i] < u[i - 1]);
      if (ok) c = u;
    }
    return c;
  }();
  return cuts;
}
int Model::backward_G_parts() const { return (int)grad_cuts().size() + 1; }

void Model::backward_G_part(float label_real, int part, size_t* ready_off, size_t* ready_count, bool join) {
  const int np = backward_G_parts();
  if (part < 0 || part >= np) throw Error(1, "backward_G_part: part out of range");
  size_t hi_off = arenaG.n, lo_off = 0;
  int hi_op = (int)G->ops.size(), lo_op = 0;
  const std::vector<double> cuts = grad_cuts();
  if (part > 0) hi_op = G->split_point(cuts[part - 1], &hi_off);
  if (part < np - 1) lo_op = G->split_point(cuts[part], &lo_off);
  if (part == 0) {
    backward_G_head(label_real);
    G->refresh_dgrad();
  }
  G->backward_range(true, false, lo_op, hi_op, join);
  if (ready_off) *ready_off = lo_off;
  if (ready_count) *ready_count = hi_off - lo_off;
}

// ---------------------------------------------------------------------------------------
AdamWArgs Model::optimizer_args(int net) {
  const ParamArena& A = arena(net);
  AdamWArgs a{};
  a.lr = net == 0 ? hyper.lr : hyper.d_lr;
  a.weight_decay = net == 0 ? hyper.weight_decay : hyper.d_weight_decay;
  a.beta1 = net == 0 ? hyper.b1 : hyper.d_b1; a.beta2 = net == 0 ? hyper.b2 : hyper.d_b2; a.eps = 1e-8f;
  a.kind = A.opt_kind;
  if (a.kind == OPT_ADAMW) {
    if (indirect) a.sched_dev = net == 0 ? sp_dev->schedG : sp_dev->schedD;
    return a;
  }
  if (a.kind != OPT_ADABOUND) throw Error(1, "optimizer_step: unknown optimizer kind");
  // the simulator's adamw_step knows AdamW only and would apply it whatever `kind` says
  if (!is_device_build()) throw Error(1, "optimizer_step: AdaBound is not implemented on the host simulator (HIP kernel only)");
  a.final_lr = A.final_lr; a.base_lr = A.base_lr; a.gamma = A.gamma;
  if (indirect) a.sched_dev = net == 0 ? sp_dev->boundG : sp_dev->boundD;
  return a;
}

void Model::optimizer_step(int net) {
  ParamArena& A = arena(net);
  AdamWArgs a = optimizer_args(net);
  A.step += 1;
  a.p = A.w; a.g = A.g; a.m = A.m; a.v = A.v; a.n = A.n;
  a.step = A.step;
  adamw_step(ctx->s, a);
  A.version += 1;
}

Net::BNBuffers Model::bn_site(const std::string& name, int C, int net) {
  for (BNSite& s : bn_sites(net))
    if (s.name == name) {
      if (s.C != C) throw Error(1, "BatchNorm site " + name + ": channel count differs from the arena owner's");
      return s.run;
    }
  if (share_) throw Error(1, "shared model: the arena's owner has no BatchNorm site " + name);
  bn_sites_[net].emplace_back();
  BNSite& s = bn_sites_[net].back();
  s.name = name; s.C = C; s.ones.assign(C, 1.f);
  float* buf = static_cast<float*>(ctx->alloc((size_t)2 * C * sizeof(float) + 16));      // zero-filled: mean 0, count 0
  s.run = Net::BNBuffers{buf, buf + C, reinterpret_cast<long long*>(buf + 2 * C)};
  dev_upload(ctx->s, s.run.var, s.ones.data(), C * sizeof(float));
  return s.run;
}
PatchganNorm Model::d_norm(int groups) {
  PatchganNorm n;
  n.kind = d_norm_; n.groups = groups;
  n.site = [this](const std::string& name, int C) { return bn_site(name, C); };
  return n;
}

void Model::discriminate(const float* x_nchw, float* pred_nchw) {
  if (!is_train || !D2) throw Error(1, "discriminate: the model has no discriminator (created with is_train = 0)");
  if (d_cimap_.empty()) throw Error(1, "discriminate: model did not publish its conditional-input channel map");
  if (!D3_) {
    AllocScope mine(*ctx, owned_allocs);
    D3_ = std::make_unique<Net>(*ctx, arenaD);
    d3_in_ = D3_->alloc_var(B, H, W, (int)d_cimap_.size(), false);
    d3_pred_ = build_patchgan(*D3_, d3_in_, d_layers_, d_cimap_, 0, d_norm(1));
    D3_->finalize({});
  }
  // scatter the reference-ordered channels into the buffer order: maximal runs of consecutive channels
  const int nb = (int)d_cimap_.size();
  const size_t plane = (size_t)H * W;
  int nref = 0;
  for (int v : d_cimap_) nref += v >= 0;
  for (int b0 = 0; b0 < nb;) {
    if (d_cimap_[b0] < 0) { ++b0; continue; }
    int len = 1;
    while (b0 + len < nb && d_cimap_[b0 + len] == d_cimap_[b0] + len) ++len;
    // NCHW source with nref channels: a channel sub-range is strided per image -> copy image by image
    for (int n = 0; n < B; ++n) {
      // (pad channels of the buffer stay zero: dev_alloc zero-fills and nothing else writes them)
      nchw_to_nhwc(ctx->s, x_nchw + ((size_t)n * nref + d_cimap_[b0]) * plane, 1, len, H, W, d3_in_.batch(n, 1).v.slice(b0, len));
    }
    b0 += len;
  }
  D3_->training = false;
  D3_->bn_training = discriminate_training;
  D3_->refresh_dgrad();
  D3_->forward();
  nhwc_to_nchw(ctx->s, d3_pred_.v, pred_nchw, 1);
}
void Model::set_gp_random(const float* alpha_dev, const float* beta_nchw_dev) {
  if (!is_train || d_cimap_.empty()) throw Error(1, "set_gp_random: the model has no discriminator");
  if (!gp_) {
    AllocScope mine(*ctx, owned_allocs); gp_ = std::make_unique<GradPenalty>(*ctx, arenaD, B, H, W, d_layers_, d_norm(1));
  }
  if (alpha_dev) { dev_copy(ctx->s, gp_->alpha_buffer(), alpha_dev, (size_t)B * sizeof(float)); gp_alpha_set_ = true; }
  if (beta_nchw_dev) {                       // reference channel order (B, 22, H, W) -> buffer order, pads stay 0
    const int nb = (int)d_cimap_.size();
    const size_t plane = (size_t)H * W;
    int nref = 0;
    for (int v : d_cimap_) nref += v >= 0;
    const TView bv = gp_->beta_buffer();
    for (int b0 = 0; b0 < nb;) {
      if (d_cimap_[b0] < 0) { ++b0; continue; }
      int len = 1;
      while (b0 + len < nb && d_cimap_[b0 + len] == d_cimap_[b0] + len) ++len;
      for (int n = 0; n < B; ++n) {
        TView dst = bv; dst.p = bv.p + (size_t)n * plane * bv.cs; dst.N = 1;
        nchw_to_nhwc(ctx->s, beta_nchw_dev + ((size_t)n * nref + d_cimap_[b0]) * plane, 1, len, H, W, dst.slice(b0, len));
      }
      b0 += len;
    }
    gp_beta_set_ = true;
  }
}
void Model::run_gradient_penalty(const TView& real, const TView& fake) {
  if (!gp_) {
    AllocScope mine(*ctx, owned_allocs); gp_ = std::make_unique<GradPenalty>(*ctx, arenaD, B, H, W, d_layers_, d_norm(1));
  }
  const TView beta = gp_->beta_buffer();
  // library RNG: a function of the step seed the caller handed to forward() (torch.initial_seed(), the step counter and --
  // under data parallelism -- the rank: every rank draws its own alpha / beta) and of the optimizer step
  const uint64_t gp_seed = (G ? G->seed : 0) * 0x9E3779B97F4A7C15ull + (uint64_t)arenaD.step * 7919ull + 13ull;
  gp_->run(real, fake, hyper.gp_mode, hyper.grad_scale, hyper.lambda_gp, gp_alpha_set_ ? gp_->alpha_buffer() : nullptr,
           gp_beta_set_ ? &beta : nullptr, gp_seed, losses + L_D_GP);
  gp_alpha_set_ = gp_beta_set_ = false;
  scalar_axpby(ctx->s, losses + L_D, 1.f, losses + L_D_GP, 1.f, losses + L_D);     // loss_D += loss_D_gp (warp_model.py:136)
}
void Model::set_style_context(const float*, const float*, int, int) {
  throw Error(1, "set_style_context: only the texture model has a style term");
}
void Model::set_input_texture_batch(const uint8_t*, int, int, int, const uint8_t*, int, int, const float*, int, const float*, const float*,
                                    const float*, int, int) {
  throw Error(1, "set_input_texture_batch: only the texture model takes a texture batch");
}
void Model::set_input_texture_sources(const uint8_t*, size_t, const int64_t*, int, int, int, const uint8_t*, int, int, const float*, int,
                                      const float*, const float*, const float*, int, int) {
  throw Error(1, "set_input_texture_sources: only the texture model takes a texture batch");
}
void Model::set_input_warp_batch(const uint8_t*, int, int, int, const uint8_t*, const uint8_t*, int, int, const double*, int, const float*,
                                 const float*, int, int, int, int) {
  throw Error(1, "set_input_warp_batch: only the warp model takes a warp batch");
}
void Model::perceptual(const float*, const float*, int, float*, float, float, float*) {
  throw Error(1, "perceptual: only the texture model carries the VGG16 network (not implemented for this model)");
}

void Model::optimizer_step_range(int net, size_t off, size_t count, int first) { optimizer_step_range_on(ctx->s, net, off, count, first); }
void Model::optimizer_step_range_on(Stream& st, int net, size_t off, size_t count, int first) {
  ParamArena& A = arena(net);
  if (off % 4 || off + count > A.n) throw Error(1, "optimizer_step_range: range outside the arena / not 16-byte aligned");
  AdamWArgs a = optimizer_args(net);
  if (first) A.step += 1;
  if (count == 0) return;
  a.p = A.w + off; a.g = A.g + off; a.m = A.m + off; a.v = A.v + off; a.n = (count + 3) / 4 * 4 <= A.n - off ? (count + 3) / 4 * 4 : count;
  a.step = A.step;
  adamw_step(st, a);
  A.version += 1;
}

void Model::backward_G_streamed(float label_real) {
  const int np = backward_G_parts();
  const int ver = arenaG.version;
  for (int part = 0; part < np; ++part) {
    size_t off = 0, count = 0;
    backward_G_part(label_real, part, &off, &count, /*join=*/false);
    // the side stream already carries the bucket's weight gradients; the fork orders it behind the bucket's main-stream work
    // too (bias sums, the input-gradient chain that produced their operands).  Nothing later on either stream reads the
    // bucket's weights or gradients again this step: the earlier layers multiply by their own (derived) operands.
    Stream& sd = ctx->use_side() ? ctx->fork_side() : ctx->s;
    optimizer_step_range_on(sd, 0, off, count, part == 0);
  }
  arenaG.version = ver + 1;      // one optimizer step
  ctx->join_side();
}

// BaseGAN.optimize_parameters as a recorded launch sequence (engine.h Model::step_captured)
void Model::step_captured(const float labels[3], bool training, uint64_t seed) {
  static_assert(sizeof(StepParams) == 64 && offsetof(StepParams, schedG) == 24 && offsetof(StepParams, schedD) == 32 &&
                offsetof(StepParams, boundG) == 40 && offsetof(StepParams, boundD) == 52, "StepParams layout (64 bytes allocated)");
  if (hyper.gp_mode) { step(labels, training, seed); return; }          // host-seeded draws per step: not recordable
  if (!sp_dev) { AllocScope mine(*ctx, owned_allocs); sp_dev = static_cast<StepParams*>(ctx->alloc(64)); }
  StepParams h{};
  for (int i = 0; i < 3; ++i) h.labels[i] = labels[i];
  h.seed = seed;
  adamw_schedule(hyper.lr, hyper.b1, hyper.b2, arenaG.step + 1, h.schedG);
  adamw_schedule(hyper.d_lr, hyper.d_b1, hyper.d_b2, arenaD.step + 1, h.schedD);
  if (arenaG.opt_kind == OPT_ADABOUND)
    adabound_schedule(hyper.lr, hyper.b1, hyper.b2, arenaG.final_lr, arenaG.base_lr, arenaG.gamma, arenaG.step + 1, h.boundG);
  if (arenaD.opt_kind == OPT_ADABOUND)
    adabound_schedule(hyper.d_lr, hyper.d_b1, hyper.d_b2, arenaD.final_lr, arenaD.base_lr, arenaD.gamma, arenaD.step + 1, h.boundD);
  dev_store_small(ctx->s, sp_dev, &h, sizeof h);      // stream-ordered, in front of this step's launches, and NO host sync (round 5: the
                                                      // synchronising upload made every replayed step wait for the previous one to drain)
  struct Indirect {
    Model& m;
    explicit Indirect(Model& mm) : m(mm) { m.indirect = true; if (m.G) m.G->seed_dev = &m.sp_dev->seed; }
    ~Indirect() { m.indirect = false; if (m.G) m.G->seed_dev = nullptr; }
  } scope(*this);
  const int gi = training ? 1 : 0;
  if (!is_device_build() || step_warm_[gi] == 0) {      // first call (and the host simulator): the phases, eagerly, on the device block
    step(labels, training, seed);
    step_warm_[gi] = 1;
    return;
  }
  // a recorded sequence bakes in what is not in StepParams: one stream or two, and where AdamW sits (round-4 advice)
  // ... and which update kernel each network's optimizer launches (the arenas, and so the kinds, may be shared with other models)
  const int key = (ctx->use_side() ? 1 : 0) | (env_int(getenv("SWN_STREAM_ADAMW"), 1) << 1) | (arenaG.opt_kind << 8) | (arenaD.opt_kind << 12);
  if (step_graph_[gi] && step_graph_key_[gi] != key) { graph_destroy(step_graph_[gi]); step_graph_[gi] = nullptr; }
  if (!step_graph_[gi]) {
    step_graph_key_[gi] = key;
    // record: the same phases on a private capture stream (the side stream joins the capture through the fork / join events)
    stream_sync(ctx->s);
    Stream& s = ctx->s;
    void* caller = s.handle;
    if (!cap_stream_) cap_stream_ = stream_create_current();
    const int stepG = arenaG.step, stepD = arenaD.step, verG = arenaG.version, verD = arenaD.version;
    s.handle = cap_stream_;
    try {
      graph_begin(s);
      try {
        step(labels, training, seed);
        ctx->join_side();
      } catch (...) { graph_abort(s); throw; }
      step_graph_[gi] = graph_end(s);
    } catch (...) { s.handle = caller; throw; }
    s.handle = caller;
    // recording executed nothing: undo the host-side bookkeeping of the recorded pass, the replay below redoes it
    arenaG.step = stepG; arenaD.step = stepD; arenaG.version = verG; arenaD.version = verD;
  }
  graph_launch(step_graph_[gi], ctx->s);
  if (!hyper.warp_mode_ce_only) { arenaD.step += 1; arenaD.version += 1; }
  arenaG.step += 1; arenaG.version += 1;
}

// Data-parallel optimize_parameters with the library's own exchange (engine.h Model::step_dp)
void Model::step_dp(const float labels[3], bool training, uint64_t seed, bool after_forward) {
  if (!ctx->comm_fn) throw Error(1, "step_dp: no communicator attached (swn_ctx_attach_comm)");
  if (!after_forward) forward(training, seed);
  if (!hyper.warp_mode_ce_only) {
    backward_D(labels[0], labels[1]);            // ends joined: every D gradient is ordered on the main stream
    // D's update precedes the D pass of backward_G by data dependence (base_gan.py:199): this exchange is serial
    Stream& cs = ctx->comm_fork();
    ctx->all_reduce_sum(cs, arenaD.g, arenaD.n);
    ctx->comm_join();
    optimizer_step(1);
  }
  const int np = backward_G_parts();
  const int ver = arenaG.version;
  for (int part = 0; part < np; ++part) {
    size_t off = 0, count = 0;
    backward_G_part(labels[2], part, &off, &count, /*join=*/true);      // the bucket's weight gradients are final on the main stream
    // exchange stream: after the bucket's gradients, behind the previous bucket's all-reduce and AdamW (stream order).  Nothing
    // later on the compute streams reads this bucket's weights or gradients again this step (backward_G_streamed's argument):
    // the earlier layers multiply by their own derived operands, which are refreshed from the weights at the next forward --
    // after the join below.
    Stream& cs = ctx->comm_fork();
    ctx->all_reduce_sum(cs, arenaG.g + off, count);
    optimizer_step_range_on(cs, 0, off, count, part == 0);
  }
  arenaG.version = ver + 1;        // one optimizer step
  ctx->comm_join();
}

// BaseGAN.optimize_parameters (models/base_gan.py:194-203): forward, D step, G step.
void Model::step(const float labels[3], bool training, uint64_t seed) {
  forward(training, seed);
  if (!hyper.warp_mode_ce_only) {
    backward_D(labels[0], labels[1]);
    optimizer_step(1);
  }
  // SWN_STREAM_ADAMW=0: AdamW as one launch behind the whole backward pass; 2: the bucketed order also without a side stream
  // (what the host simulator can exercise).  Read per step.
  const int mode = env_int(getenv("SWN_STREAM_ADAMW"), 1);
  if (mode == 2 || (mode != 0 && ctx->use_side())) {
    backward_G_streamed(labels[2]);
    return;
  }
  backward_G(labels[2]);
  optimizer_step(0);
}

// Host fallbacks of the BatchNorm launchers (ops.h).  Weak: the device library links batch_norm.hip, whose definitions take their
// place; the host simulator has none, so a BatchNorm site there fails with the library's "not implemented" error.
__attribute__((weak)) void batch_norm_fwd(Stream&, const BatchNormArgs&) {
  throw Error(1, "batch_norm_fwd: BatchNorm is not implemented on the host simulator (HIP kernel only)");
}
__attribute__((weak)) void batch_norm_bwd(Stream&, const BatchNormBwdArgs&) {
  throw Error(1, "batch_norm_bwd: BatchNorm is not implemented on the host simulator (HIP kernel only)");
}
__attribute__((weak)) void batch_norm_bwd2(Stream&, const BatchNormBwd2Args&) {
  throw Error(1, "batch_norm_bwd2: BatchNorm is not implemented on the host simulator (HIP kernel only)");
}
__attribute__((weak)) void time_launches(Stream&, int, int, const std::function<void()>&, float*) {
  throw Error(1, "time_launches: device timing is not implemented on the host simulator");
}

// Host form of the texture batch hand-over (ops.h texture_batch).  Weak like the fallbacks above, but a real implementation: the
// same expressions in the same order as texture_batch.hip, so the host simulator hands batches over too.
__attribute__((weak)) void texture_batch(Stream&, const TextureBatchArgs& a) {
  texture_batch_check(a);
  const int B = a.in_tex.N, H = a.in_tex.H, W = a.in_tex.W, Cp = round_up(a.C, 4);
  const bool clamp_rois = !(a.x_min == 0 && a.y_min == 0 && H == a.Hs && W == a.Ws);
  const float lscale_y = (float)a.Hl / (float)a.Hs, lscale_x = (float)a.Wl / (float)a.Ws;
  auto texel = [&](const uint8_t* px, float* dst) {
    for (int c = 0; c < 3; ++c) {
      volatile float t = (float)px[c] / 255.f;           // (volatile: one rounded fp32 operation per step, whatever the compiler's contraction rules)
      volatile float d = t - a.mean[c];
      dst[c] = d / a.std[c];
    }
    dst[3] = 0.f;
  };
  for (int b = 0; b < B; ++b) {
    const float* sp = a.sample + (size_t)b * 5;
    const bool vf = sp[0] != 0.f, hf = sp[1] != 0.f;
    const uint8_t* im = a.img + (size_t)b * a.Hs * a.Ws * 3;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t pix = ((size_t)b * H + y) * W + x;
        const int sy = a.y_min + y, sx = a.x_min + x;
        const int fy = vf ? a.Hs - 1 - sy : sy, fx = hf ? a.Ws - 1 - sx : sx;
        texel(im + ((size_t)fy * a.Ws + fx) * 3, a.in_tex.p + pix * a.in_tex.cs);
        if (a.tgt_tex.p) texel(im + ((size_t)sy * a.Ws + sx) * 3, a.tgt_tex.p + pix * a.tgt_tex.cs);
        const int ly = std::min((int)floorf((float)sy * lscale_y), a.Hl - 1), lx = std::min((int)floorf((float)sx * lscale_x), a.Wl - 1);
        const int l = a.labels[((size_t)b * a.Hl + ly) * a.Wl + lx];
        for (int k = 0; k < a.ncloth; ++k) {
          float* dst = a.cloth[k].p + pix * a.cloth[k].cs;
          for (int c = 0; c < Cp; ++c) dst[c] = (c == l && l != 0 && l < a.C) ? 1.f : 0.f;
        }
      }
    auto mirror = [](float v, float c) { volatile float d = v - c; return -d + c; };
    auto crop1 = [](float v, float lo, float hi) { return std::fmin(std::fmax(v, lo), hi) - lo; };
    for (int r = 0; r < a.R; ++r) {
      const float* raw = a.rois_raw + ((size_t)b * a.R + r) * 4;
      float* out = a.rois_out + ((size_t)b * a.R + r) * 4;
      float v[4];
      for (int j = 0; j < 4; ++j) { volatile float m = raw[j] * sp[2]; v[j] = rintf(m); }
      if (vf) { const float lo = mirror(v[3], sp[3]), hi = mirror(v[1], sp[3]); v[1] = lo; v[3] = hi; }      // vertical first
      if (hf) { const float lo = mirror(v[2], sp[4]), hi = mirror(v[0], sp[4]); v[0] = lo; v[2] = hi; }
      if (clamp_rois) {
        const float xl = (float)a.x_min, xh = (float)(a.x_min + W - 1), yl = (float)a.y_min, yh = (float)(a.y_min + H - 1);
        v[0] = crop1(v[0], xl, xh); v[2] = crop1(v[2], xl, xh); v[1] = crop1(v[1], yl, yh); v[3] = crop1(v[3], yl, yh);
      }
      for (int j = 0; j < 4; ++j) out[j] = v[j];
    }
  }
}

// Host form of chain_resample.h's chain_value (ops.h chain_resample): one chain at one output pixel, the same expressions in the same
// order, a tap at a time instead of the sixteen together.  src(index) is the image's value at flat index y * W + x.
namespace {
template <class Src>
float chain_value_host(const double* rows, int nmaps, int x0, int y0, int W, int H, Src src) {
  // (volatile: one rounded operation per step, whatever the compiler's contraction rules)
  auto dadd = [](double x, double y) { volatile double r = x + y; return (double)r; };
  auto dsub = [](double x, double y) { volatile double r = x - y; return (double)r; };
  auto dmul = [](double x, double y) { volatile double r = x * y; return (double)r; };
  auto fadd = [](float x, float y) { volatile float r = x + y; return (float)r; };
  auto fsub = [](float x, float y) { volatile float r = x - y; return (float)r; };
  auto fmul = [](float x, float y) { volatile float r = x * y; return (float)r; };
  auto pil_floor = [](double v) { return v < 0.0 ? (int)std::floor(v) : (int)v; };
  auto perspective_src = [&](const double* m, long long x, long long y, double& fx, double& fy) {
    const double xc = (double)x + 0.5, yc = (double)y + 0.5;
    const double den = dadd(dadd(dmul(m[7], xc), dmul(m[8], yc)), 1.0);
    fx = dadd(dadd(dmul(m[1], xc), dmul(m[2], yc)), m[3]) / den;
    fy = dadd(dadd(dmul(m[4], xc), dmul(m[5], yc)), m[6]) / den;
  };
  auto nearest_step = [&](const double* m, long long& x, long long& y) {
    const int kind = (int)m[0];
    long long xin = x, yin = y;
    if (kind == 1) {
      xin = ((long long)m[3] + (long long)m[2] * y + (long long)m[1] * x) >> 16;
      yin = ((long long)m[6] + (long long)m[5] * y + (long long)m[4] * x) >> 16;
    } else if (kind == 2 || kind == 3) {
      double fx, fy;
      perspective_src(m, x, y, fx, fy);
      xin = fx < 0.0 ? -1 : (long long)(int)fx;
      yin = fy < 0.0 ? -1 : (long long)(int)fy;
    }
    x = xin; y = yin;
    return xin >= 0 && xin < W && yin >= 0 && yin < H;
  };
  auto horner = [&](double p1, double p2, double p3, double p4, double d) {
    return dadd(p1, dmul(d, dadd(p2, dmul(d, dadd(p3, dmul(d, p4))))));
  };
  auto cubic_taps = [&](float v1, float v2, float v3, float v4, double d) {
    return horner((double)v2, (double)fadd(-v1, v3), (double)fsub(fadd(fmul(2.f, fsub(v1, v2)), v3), v4),
                  (double)fadd(fsub(fadd(-v1, v2), v3), v4), d);
  };
  auto cubic_rows = [&](double v1, double v2, double v3, double v4, double d) {
    return horner(v2, dadd(-v1, v3), dsub(dadd(dmul(2.0, dsub(v1, v2)), v3), v4), dadd(dsub(dadd(-v1, v2), v3), v4), d);
  };
  long long x = x0, y = y0;
  int k = nmaps - 1;
  for (; k >= 0; --k) {
    const double* m = rows + (size_t)k * 9;
    if ((int)m[0] == 3) break;
    if (!nearest_step(m, x, y)) return 0.f;
  }
  if (k < 0) return src((int)y * W + (int)x);
  double fx, fy;
  perspective_src(rows + (size_t)k * 9, x, y, fx, fy);
  const int ix = pil_floor(fx), iy = pil_floor(fy);
  if (ix < 0 || ix >= W || iy < 0 || iy >= H) return 0.f;
  fx = dsub(fx, 0.5); fy = dsub(fy, 0.5);
  const int wx = pil_floor(fx), wy = pil_floor(fy);
  const double dx = dsub(fx, (double)wx), dy = dsub(fy, (double)wy);
  auto tap = [&](int tx, int ty) {                         // through the rows in front of the kind-3 row; 0 where it leaves the image
    long long px = tx, py = ty;
    for (int r = k - 1; r >= 0; --r)
      if (!nearest_step(rows + (size_t)r * 9, px, py)) return 0.f;
    return (float)src((int)py * W + (int)px);
  };
  double rv[4];
  for (int j = 0; j < 4; ++j) {
    const int yy = wy - 1 + j;
    if (j > 0 && !(yy >= 0 && yy < H)) { rv[j] = rv[j - 1]; continue; }
    const int yc = std::min(std::max(yy, 0), H - 1);
    float v[4];
    for (int i = 0; i < 4; ++i) v[i] = tap(std::min(std::max(wx - 1 + i, 0), W - 1), yc);
    rv[j] = cubic_taps(v[0], v[1], v[2], v[3], dx);
  }
  return (float)cubic_rows(rv[0], rv[1], rv[2], rv[3], dy);
}
}  // namespace

// Host form of ops.h chain_resample, weak like texture_batch above.
__attribute__((weak)) void chain_resample(Stream&, const float* src, float* dst, int B, int C, int H, int W, const double* maps, int nmaps) {
  chain_resample_check(B, C, H, W, nmaps);
  for (int bc = 0; bc < B * C; ++bc) {
    const float* img = src + (size_t)bc * H * W;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        dst[((size_t)bc * H + y) * W + x] = chain_value_host(maps + (size_t)bc * nmaps * 9, nmaps, x, y, W, H, [&](int idx) { return img[idx]; });
  }
}

// Host form of the warp batch hand-over (ops.h warp_batch), weak like texture_batch above: the same expressions in the same order as
// warp_batch.hip.
__attribute__((weak)) void warp_batch(Stream&, const WarpBatchArgs& a) {
  warp_batch_check(a);
  const int B = a.in_cloth.N, H = a.in_cloth.H, W = a.in_cloth.W, Cp = round_up(a.C, 4), nmaps = a.maps ? a.nmaps : 0;
  const float lscale_y = (float)a.Hl / (float)a.Ls, lscale_x = (float)a.Wl / (float)a.Ls;
  const float bscale_y = (float)a.Hb / (float)a.Ls, bscale_x = (float)a.Wb / (float)a.Ls;
  // (volatile: one rounded fp32 operation per step, whatever the compiler's contraction rules)
  auto mul = [](float x, float y) { volatile float r = x * y; return (float)r; };
  auto add = [](float x, float y) { volatile float r = x + y; return (float)r; };
  auto sub = [](float x, float y) { volatile float r = x - y; return (float)r; };
  auto texel = [&](const uint8_t* px, int c) { volatile float t = (float)px[c] / 255.f; volatile float d = t - a.mean[c]; return d / a.std[c]; };
  auto bilinear_src = [&](int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = std::fmax(sub(mul(scale, (float)dst + 0.5f), 0.5f), 0.f);
    i0 = std::min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = sub(src, (float)i0);
    l0 = sub(1.f, l1);
  };
  auto walk = [&](int bc, int x0, int y0) {                   // affine_gather's walk: the source pixel's index, or -1 outside
    long long x = x0, y = y0;
    for (int k = nmaps - 1; k >= 0; --k) {
      const double* m = a.maps + ((size_t)bc * nmaps + k) * 9;
      const int kind = (int)m[0];
      long long xin = x, yin = y;
      if (kind == 1) {
        xin = ((long long)m[3] + (long long)m[2] * y + (long long)m[1] * x) >> 16;
        yin = ((long long)m[6] + (long long)m[5] * y + (long long)m[4] * x) >> 16;
      } else if (kind == 2) {
        const double xc = (double)x + 0.5, yc = (double)y + 0.5;
        const double den = m[7] * xc + m[8] * yc + 1.0;
        const double fx = (m[1] * xc + m[2] * yc + m[3]) / den, fy = (m[4] * xc + m[5] * yc + m[6]) / den;
        xin = fx < 0.0 ? -1 : (long long)(int)fx;
        yin = fy < 0.0 ? -1 : (long long)(int)fy;
      }
      if (!(xin >= 0 && xin < a.Wl && yin >= 0 && yin < a.Hl)) return -1;
      x = xin; y = yin;
    }
    return (int)y * a.Wl + (int)x;
  };
  for (int b = 0; b < B; ++b) {
    const uint8_t* im = a.body + (size_t)b * a.Hb * a.Wb * 3;
    const size_t lb = (size_t)b * a.Hl * a.Wl;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t pix = ((size_t)b * H + y) * W + x;
        const int sy = a.y_min + y, sx = a.x_min + x;
        int y0, y1, x0, x1; float h0, h1, w0, w1;
        bilinear_src(sy, bscale_y, a.Hb, y0, y1, h0, h1);
        bilinear_src(sx, bscale_x, a.Wb, x0, x1, w0, w1);
        const uint8_t* pa = im + ((size_t)y0 * a.Wb + x0) * 3; const uint8_t* pb = im + ((size_t)y0 * a.Wb + x1) * 3;
        const uint8_t* pc = im + ((size_t)y1 * a.Wb + x0) * 3; const uint8_t* pd = im + ((size_t)y1 * a.Wb + x1) * 3;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < 3; ++c) {
          const float top = add(mul(w0, texel(pa, c)), mul(w1, texel(pb, c)));
          const float bot = add(mul(w0, texel(pc, c)), mul(w1, texel(pd, c)));
          v[c] = add(mul(h0, top), mul(h1, bot));
        }
        for (int k = 0; k < a.nbody; ++k)
          for (int c = 0; c < 4; ++c) a.body_out[k].p[pix * a.body_out[k].cs + c] = v[c];
        const int ly = std::min((int)floorf(mul((float)sy, lscale_y)), a.Hl - 1), lx = std::min((int)floorf(mul((float)sx, lscale_x)), a.Wl - 1);
        if (a.tgt_cloth.p) {
          const int l = a.tgt_labels[lb + (size_t)ly * a.Wl + lx];
          float* dst = a.tgt_cloth.p + pix * a.tgt_cloth.cs;
          for (int c = 0; c < Cp; ++c) dst[c] = (c == l && l != 0 && l < a.C) ? 1.f : 0.f;
        }
        float* dst = a.in_cloth.p + pix * a.in_cloth.cs;
        for (int c = 0; c < Cp; ++c) {
          dst[c] = 0.f;
          if (c == 0 || c >= a.C) continue;
          if (a.bicubic) {                               // the table may hold kind 3: the chain by chain_resample's rule on the indicators
            auto hot = [&](int idx) { return a.in_labels[lb + idx] == c ? 1.f : 0.f; };
            dst[c] = nmaps ? chain_value_host(a.maps + (size_t)(b * a.C + c) * nmaps * 9, nmaps, lx, ly, a.Wl, a.Hl, hot) : hot(ly * a.Wl + lx);
            continue;
          }
          const int src = walk(b * a.C + c, lx, ly);
          if (src >= 0 && a.in_labels[lb + src] == c) dst[c] = 1.f;
        }
      }
  }
}

// Host form of Pillow's bilinear resize (ops.h resize_u8), weak like texture_batch above: the same expressions in the same order as
// image_resize.hip, whole images instead of tiles.
__attribute__((weak)) void resize_u8(Stream&, const ResizeU8Args& a) {
  resize_u8_check(a);
  struct Axis { std::vector<int> kmin, kn, k; int ksize = 1; };
  auto tri = [](double v) { if (v < 0.0) v = -v; return v < 1.0 ? 1.0 - v : 0.0; };
  // (volatile: one rounded double operation per step, whatever the compiler's contraction rules)
  auto windows = [&](int in, int out) {
    Axis ax;
    ax.kmin.resize(out); ax.kn.resize(out);
    if (in == out) {                                           // not resampled: the identity window returns the byte exactly
      ax.k.assign(out, 1 << 22);
      for (int xx = 0; xx < out; ++xx) { ax.kmin[xx] = xx; ax.kn[xx] = 1; }
      return ax;
    }
    volatile double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : (double)scale;
    volatile double support = 1.0 * fs;
    volatile double ss = 1.0 / fs;
    ax.ksize = 2 * RESIZE_MAX_FACTOR + 2;
    ax.k.assign((size_t)out * ax.ksize, 0);
    for (int xx = 0; xx < out; ++xx) {
      volatile double center = ((double)xx + 0.5) * scale;
      volatile double lo = center - support;
      volatile double hi = center + support;
      int xmin = (int)(lo + 0.5);
      if (xmin < 0) xmin = 0;
      int xmax = (int)(hi + 0.5);
      if (xmax > in) xmax = in;
      const int n = std::min(xmax - xmin, ax.ksize);
      int* k = ax.k.data() + (size_t)xx * ax.ksize;
      volatile double ww = 0.0;
      for (int x = 0; x < n; ++x) {
        volatile double d = (double)(x + xmin) - center;
        volatile double e = d + 0.5;
        volatile double arg = e * ss;
        ww = ww + tri(arg);
      }
      for (int x = 0; x < n; ++x) {
        volatile double d = (double)(x + xmin) - center;
        volatile double e = d + 0.5;
        volatile double arg = e * ss;
        volatile double w = tri(arg);
        if (ww != 0.0) w = w / ww;
        volatile double q = w * 4194304.0;
        k[x] = (int)(0.5 + q);
      }
      ax.kmin[xx] = xmin; ax.kn[xx] = n;
    }
    return ax;
  };
  auto clip8 = [](int acc) { const int v = acc >> 22; return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
  std::vector<uint8_t> inter;
  for (int b = 0; b < a.B; ++b) {
    const int H0 = (int)a.geom[3 * b + 1], W0 = (int)a.geom[3 * b + 2];
    const uint8_t* im = a.src + a.geom[3 * b];
    uint8_t* out = a.dst + (size_t)b * a.Hs * a.Ws * 3;
    const Axis hx = windows(W0, a.Ws), vx = windows(H0, a.Hs);
    inter.resize((size_t)H0 * a.Ws * 3);
    for (int y = 0; y < H0; ++y)                               // horizontal pass: rounded bytes (H0, Ws)
      for (int x = 0; x < a.Ws; ++x)
        for (int c = 0; c < 3; ++c) {
          const uint8_t* sp = im + ((size_t)y * W0 + hx.kmin[x]) * 3 + c;
          const int* k = hx.k.data() + (size_t)x * hx.ksize;
          int acc = 1 << 21;
          for (int i = 0; i < hx.kn[x]; ++i) acc += (int)sp[(size_t)i * 3] * k[i];
          inter[((size_t)y * a.Ws + x) * 3 + c] = clip8(acc);
        }
    const size_t rowlen = (size_t)a.Ws * 3;
    for (int y = 0; y < a.Hs; ++y) {                           // vertical pass on those
      const int* k = vx.k.data() + (size_t)y * vx.ksize;
      for (size_t j = 0; j < rowlen; ++j) {
        int acc = 1 << 21;
        for (int i = 0; i < vx.kn[y]; ++i) acc += (int)inter[(size_t)(vx.kmin[y] + i) * rowlen + j] * k[i];
        out[(size_t)y * rowlen + j] = clip8(acc);
      }
    }
  }
}

// Host form of the saved-image visuals (ops.h image_u8), weak like texture_batch above: the same expressions in the same order as
// image_out.hip, whole images instead of four-pixel groups; the min / max of scale_each is taken in place (the scratch is not used).
__attribute__((weak)) void image_u8(Stream&, const ImageU8Args& args) {
  const ImageU8Args a = image_u8_check(args);
  static const uint8_t palette[LABEL_PALETTE_SIZE][3] = {SWN_LABEL_PALETTE};
  const int HW = a.H * a.W, w = a.width;
  // (volatile: one rounded fp32 operation per step, whatever the compiler's contraction rules)
  auto to_byte = [&](float u) {
    float t;
    if (a.range == RANGE_SIGNED) { volatile float s1 = u + 1.f; volatile float h = s1 / 2.f; volatile float m = h * 255.f; t = m; }
    else { volatile float m = u * 255.f; t = m; }
    return (uint8_t)(int)std::fmin(std::fmax(t, 0.f), 255.f);
  };
  for (int b = 0; b < a.B; ++b) {
    float lo = INFINITY, hi = -INFINITY, den = 1.f;
    if (a.scale_each) {
      for (int p = 0; p < HW; ++p)
        for (int c = 0; c < a.C; ++c) { const float v = a.x.p[((size_t)b * HW + p) * a.x.cs + c]; lo = std::fmin(lo, v); hi = std::fmax(hi, v); }
      den = (float)((double)hi - (double)lo + 1e-5);
    }
    const float* row = a.rows ? a.rows + (size_t)b * (2 * a.C + 1) : nullptr;
    int box[IMAGE_MAX_ROIS][6];
    for (int r = 0; r < a.R; ++r) {
      const float* q = a.rois + ((size_t)b * a.R + r) * 4;
      for (int j = 0; j < 4; ++j) box[r][j] = (int)std::fmin(std::fmax(q[j], -536870912.f), 536870912.f);
      const int s0 = box[r][1] + w, e = box[r][3] - w + 1;
      box[r][4] = s0 <= e ? s0 : e + 1; box[r][5] = s0 <= e ? e - 1 : s0;
    }
    for (int y = 0; y < a.H; ++y)
      for (int x = 0; x < a.W; ++x) {
        const size_t pix = (size_t)b * HW + (size_t)y * a.W + x;
        uint8_t rgb[3] = {0, 0, 0};
        if (a.source == SRC_FLOAT) {
          const float* px = a.x.p + pix * a.x.cs;
          for (int c = 0; c < 3; ++c) {
            const int cc = a.C == 1 ? 0 : c;
            float u = px[cc];
            if (row) {
              volatile float m = u * row[cc];
              volatile float s1 = m + row[a.C + cc];
              u = s1;
              if (row[2 * a.C] != 0.f) u = std::fmin(std::fmax(u, 0.f), 1.f);
            } else if (a.scale_each) {
              volatile float s1 = std::fmin(std::fmax(u, lo), hi) + (-lo);
              volatile float d = s1 / den;
              u = d;
            }
            rgb[c] = to_byte(u);
          }
        } else {
          int best = 0;
          if (a.source == SRC_LABELS) {
            best = a.labels[pix];
          } else {
            const float* px = a.x.p + pix * a.x.cs;
            float m = px[0];
            for (int c = 1; c < a.C; ++c) if (px[c] > m) { m = px[c]; best = c; }
          }
          if (best >= 0 && best < LABEL_PALETTE_SIZE) for (int c = 0; c < 3; ++c) rgb[c] = palette[best][c];
        }
        for (int r = 0; r < a.R; ++r) {
          const int x0 = box[r][0], y0 = box[r][1], x1 = box[r][2], y1 = box[r][3];
          const bool rows_hit = x >= x0 && x <= x1 && ((y >= y0 && y <= y0 + w - 1) || (y >= y1 - w + 1 && y <= y1));
          const bool cols_hit = ((x >= x0 && x <= x0 + w - 1) || (x >= x1 - w + 1 && x <= x1)) && y >= box[r][4] && y <= box[r][5];
          if (rows_hit || cols_hit) for (int c = 0; c < 3; ++c) rgb[c] = a.colours[r * 3 + c];
        }
        for (int c = 0; c < 3; ++c) a.out[pix * 3 + c] = rgb[c];
      }
  }
}

// ---- PNG encoding (ops.h png_encode) --------------------------------------------------------------------------------------------------
// The shapes the encoder takes and the sizes of its buffers: one definition for the launcher, the C interface and the pipeline.
PngGeom png_geometry(int h, int w, int rows_per_chunk) {
  if (h < 1 || w < 1) throw Error(1, "png_encode: empty image");
  if (w > PNG_MAX_WIDTH) throw Error(1, "png_encode: images wider than " + std::to_string(PNG_MAX_WIDTH) + " pixels are refused, got " + std::to_string(w));
  if (h > (1 << 24)) throw Error(1, "png_encode: images of more than 2^24 rows are refused");
  if (rows_per_chunk < 0) throw Error(1, "png_encode: rows_per_chunk must be positive, or 0 for the default");
  const int stride = 1 + 3 * w;
  PngGeom g;
  g.R = rows_per_chunk ? rows_per_chunk : std::max(1, std::min(16, PNG_MAX_CHUNK / stride));
  if ((size_t)g.R * stride > (size_t)PNG_MAX_CHUNK)
    throw Error(1, "png_encode: a chunk of " + std::to_string(g.R) + " rows of " + std::to_string(stride) + " bytes exceeds " +
                       std::to_string(PNG_MAX_CHUNK) + " bytes");
  g.R = std::min(g.R, h);
  g.chunks = (h + g.R - 1) / g.R;
  g.chunk_bytes = g.R * stride;
  g.last_bytes = (h - (g.chunks - 1) * g.R) * stride;
  g.slot = png_slot_stride((size_t)g.chunk_bytes);
  g.bound = 2 + (size_t)(g.chunks - 1) * png_chunk_cap((size_t)g.chunk_bytes) + png_chunk_cap((size_t)g.last_bytes) + 4;
  return g;
}
// Weak like the BatchNorm launchers: the device library links png_encode.hip; the host simulator refuses by name.
__attribute__((weak)) void png_encode(Stream&, const PngEncodeArgs&) {
  throw Error(1, "png_encode: PNG encoding is not implemented on the host simulator (HIP kernel only)");
}

// ---- SSIM and Charbonnier losses (ops.h ssim_loss / charbonnier_loss) -----------------------------------------------------------------
// Host forms, weak like texture_batch above: the expressions of ssim_math.h in the order ssim.hip applies them (row pass over the taps
// in index order, then the column pass; a tap outside the image adds a zero), plane by plane with whole-plane temporaries.
namespace {
// out[q] = the zero-padded separable filter of in[q], q < Q planes of H x W
void ssim_filter_planes(const SsimWindow& win, int ws, int H, int W, int Q, const std::vector<float>* in, std::vector<float>* out) {
  const int P = ws / 2;
  std::vector<float> rows((size_t)H * W);
  for (int q = 0; q < Q; ++q) {
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float v = 0.f;
        for (int k = 0; k < ws; ++k) {
          const int sx = x + k - P;
          v += win.w[k] * (sx >= 0 && sx < W ? in[q][(size_t)y * W + sx] : 0.f);
        }
        rows[(size_t)y * W + x] = v;
      }
    out[q].assign((size_t)H * W, 0.f);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float v = 0.f;
        for (int k = 0; k < ws; ++k) {
          const int sy = y + k - P;
          v += win.w[k] * (sy >= 0 && sy < H ? rows[(size_t)sy * W + x] : 0.f);
        }
        out[q][(size_t)y * W + x] = v;
      }
  }
}
}  // namespace

__attribute__((weak)) void ssim_loss(Stream&, const SsimArgs& a) {
  ssim_check(a);
  const SsimWindow win = ssim_window(a.window);
  const float C1 = ssim_c1(a.max_val), C2 = ssim_c2(a.max_val);
  const int H = a.H, W = a.W, P = a.window / 2;
  const size_t hw = (size_t)H * W;
  const bool grad = a.d1 || a.d2;
  double total = 0;
  std::vector<float> rows[5], mom[5], coef[4], fc[4];
  for (int plane = 0; plane < a.B * a.C; ++plane) {
    const float* x = a.img1 + (size_t)plane * hw;
    const float* y = a.img2 + (size_t)plane * hw;
    // row pass: the five products enter the filter tap by tap (ssim_tap), as in the kernel
    for (auto& r : rows) r.assign(hw, 0.f);
    for (int yy = 0; yy < H; ++yy)
      for (int xx = 0; xx < W; ++xx) {
        SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.window; ++k) {
          const int sx = xx + k - P;
          const bool in = sx >= 0 && sx < W;
          ssim_tap(m, win.w[k], in ? x[(size_t)yy * W + sx] : 0.f, in ? y[(size_t)yy * W + sx] : 0.f);
        }
        const size_t o = (size_t)yy * W + xx;
        rows[0][o] = m.m1; rows[1][o] = m.m2; rows[2][o] = m.e11; rows[3][o] = m.e22; rows[4][o] = m.e12;
      }
    if (grad)
      for (auto& c : coef) c.assign(hw, 0.f);
    for (int yy = 0; yy < H; ++yy)
      for (int xx = 0; xx < W; ++xx) {
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.window; ++k) {
          const int sy = yy + k - P;
          for (int q = 0; q < 5; ++q) v[q] += win.w[k] * (sy >= 0 && sy < H ? rows[q][(size_t)sy * W + xx] : 0.f);
        }
        const size_t o = (size_t)yy * W + xx;
        const SsimMoments m = {v[0], v[1], v[2], v[3], v[4]};
        const SsimTerms st = ssim_terms(m, C1, C2);
        const float l = ssim_loss_of(st.S);
        total += (double)l;
        if (a.loss_map) a.loss_map[(size_t)plane * hw + o] = l;
        if (grad) {
          const SsimCoefs c = ssim_coefs(m, st, a.gmap ? a.gmap[(size_t)plane * hw + o] : a.gscalar);
          coef[0][o] = c.a1; coef[1][o] = c.a2; coef[2][o] = c.b; coef[3][o] = c.c;
        }
      }
    if (grad) {
      ssim_filter_planes(win, a.window, H, W, 4, coef, fc);
      for (size_t o = 0; o < hw; ++o) {
        const float xv = x[o], yv = y[o];
        if (a.d1) a.d1[(size_t)plane * hw + o] = fc[0][o] + 2.f * xv * fc[2][o] + yv * fc[3][o];
        if (a.d2) a.d2[(size_t)plane * hw + o] = fc[1][o] + 2.f * yv * fc[2][o] + xv * fc[3][o];
      }
    }
  }
  a.loss_sum[0] = (float)total;
}

__attribute__((weak)) void charbonnier_loss(Stream&, const CharbonnierArgs& a) {
  if (!a.x || !a.y || !a.loss_sum) throw Error(1, "charbonnier: NULL argument");
  if (a.n < 1) throw Error(1, "charbonnier: empty input");
  double total = 0;
  for (size_t i = 0; i < a.n; ++i) {
    float gr;
    total += (double)charbonnier_term(a.x[i], a.y[i], a.eps, a.gscalar, &gr);
    if (a.dx) a.dx[i] = gr;
    if (a.dy) a.dy[i] = -gr;
  }
  a.loss_sum[0] = (float)total;
}

}  // namespace swn
