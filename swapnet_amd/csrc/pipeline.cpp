// swapnet_amd -- two-stage inference kept on the device and replayed as a hipGraph (SURVEY.md 8(f) rank 2;
// reference: inference.py:94-126 with the .npz hand-off of :140-149 / :169-180 replaced by an HBM label map).
#include "engine.h"

#include <string>
#include <vector>

namespace swn {

Pipeline::Pipeline(Model& warp, Model& texture) : warp_(warp), tex_(texture) {
  if (warp.ctx != texture.ctx) throw Error(1, "pipeline: both models must live in the same context");
  if (warp.B != texture.B || warp.H != texture.H || warp.W != texture.W)
    throw Error(1, "pipeline: warp and texture models must share (B, H, W)");
  ctx_ = warp.ctx;
  AllocScope mine(*ctx_, owned_);
  labels_ = static_cast<int32_t*>(warp.ctx->alloc((size_t)warp.B * warp.H * warp.W * sizeof(int32_t)));
}
Pipeline::~Pipeline() {
  graph_destroy(exec_);
  stream_destroy(cap_stream_);
  ctx_->release(owned_);
}

void Pipeline::enqueue() {
  Stream& s = warp_.ctx->s;
  warp_.forward(false, 0);
  argmax_labels(s, warp_.output_view(), warp_.output_channels(), labels_);
  tex_.set_input_labels(2, labels_, tex_.B, tex_.H, tex_.W);
  tex_.forward(false, 0);
  if (sheet_) enqueue_images();
}

void Pipeline::enable_images(const float body_mean[3], const float body_std[3], const float tex_mean[3], const float tex_std[3],
                             const uint8_t* colours_host, int width, bool reference_quirk) {
  const int B = warp_.B;
  int Cb = 0, R = 0;
  warp_.input_view(0, &Cb);
  tex_.staged_rois(&R);
  if (Cb != 3) throw Error(1, "pipeline images: bodys_unnormalized needs an RGB body, this warp model has " + std::to_string(Cb) + " body channels");
  if (R < 1 || R > IMAGE_MAX_ROIS) throw Error(1, "pipeline images: 1 to " + std::to_string(IMAGE_MAX_ROIS) + " ROIs per image, this texture model has " + std::to_string(R));
  if (!colours_host) throw Error(1, "pipeline images: NULL colour table");
  if (width < 1 || width > (1 << 20)) throw Error(1, "pipeline images: outline width in [1, 2^20]");
  Stream& s = ctx_->s;
  stream_sync(s);                          // a replay in flight reads the tables and the graph that are about to go
  graph_destroy(exec_); exec_ = nullptr; warmed_ = false;      // the sequence changes: eager, then capture, again
  if (!sheet_) {
    AllocScope mine(*ctx_, owned_);
    const size_t image = (size_t)B * warp_.H * warp_.W * 3;
    minmax_ = static_cast<float*>(ctx_->alloc((size_t)B * image_u8_chunks(warp_.H, warp_.W) * 2 * sizeof(float)));
    rows_ = static_cast<float*>(ctx_->alloc((size_t)2 * B * 7 * sizeof(float)));
    colours_ = static_cast<uint8_t*>(ctx_->alloc((size_t)R * 3));
    sheet_ = static_cast<uint8_t*>(ctx_->alloc(IMAGE_SHEETS * image));
  }
  // unnormalize (datasets/data_utils.py:41-58) zips over dim 0: under reference_quirk image b < 3 gets (std[b], mean[b]) on all its
  // channels and is clamped, the images behind it are left as they are; otherwise every image gets the per-channel form
  std::vector<float> rows((size_t)2 * B * 7);
  for (int t = 0; t < 2; ++t) {
    const float* mean = t ? tex_mean : body_mean; const float* sd = t ? tex_std : body_std;
    for (int b = 0; b < B; ++b) {
      float* r = rows.data() + ((size_t)t * B + b) * 7;
      for (int c = 0; c < 3; ++c) {
        r[c] = reference_quirk ? (b < 3 ? sd[b] : 1.f) : sd[c];
        r[3 + c] = reference_quirk ? (b < 3 ? mean[b] : 0.f) : mean[c];
      }
      r[6] = (!reference_quirk || b < 3) ? 1.f : 0.f;
    }
  }
  dev_upload(s, rows_, rows.data(), rows.size() * sizeof(float));
  dev_upload(s, colours_, colours_host, (size_t)R * 3);
  width_ = width;
}

void Pipeline::enqueue_images() {
  Stream& s = ctx_->s;
  const int B = warp_.B;
  const size_t image = (size_t)B * warp_.H * warp_.W * 3;
  int k = 0;
  auto base = [&] { ImageU8Args a; a.out = sheet_ + image * k++; return a; };
  { ImageU8Args a = base(); a.source = SRC_ARGMAX; a.x = warp_.input_view(1, &a.C); image_u8(s, a); }          // inputs_decoded
  { ImageU8Args a = base(); a.x = warp_.input_view(0, &a.C); a.rows = rows_; image_u8(s, a); }                  // bodys_unnormalized
  { ImageU8Args a = base(); a.source = SRC_LABELS; a.labels = labels_; a.B = B; a.H = warp_.H; a.W = warp_.W; image_u8(s, a); }   // fakes_decoded
  { ImageU8Args a = base(); a.x = tex_.input_view(0, &a.C); a.rows = rows_ + (size_t)B * 7;                     // textures_unnormalized
    a.rois = tex_.staged_rois(&a.R); a.colours = colours_; a.width = width_; image_u8(s, a); }
  { ImageU8Args a = base(); a.x = tex_.output_view(); a.C = 3; image_u8(s, a); }                                // fakes
  { ImageU8Args a = base(); a.x = tex_.output_view(); a.C = 3; a.scale_each = 1; a.minmax = minmax_; image_u8(s, a); }   // fakes_scaled
  if (png_streams_) {
    PngEncodeArgs a;
    a.img = sheet_; a.n = IMAGE_SHEETS * B; a.h = warp_.H; a.w = warp_.W; a.rows_per_chunk = png_rows_;
    a.scratch = png_scratch_; a.streams = png_streams_; a.stream_stride = png_stride_; a.sizes = png_sizes_;
    png_encode(s, a);
  }
}

void Pipeline::enable_png(int rows_per_chunk) {
  if (!sheet_) throw Error(1, "swn_pipeline_enable_png: the pipeline has no image sheet: call swn_pipeline_enable_images first");
  if (!is_device_build()) throw Error(1, "swn_pipeline_enable_png: PNG encoding is not implemented on the host simulator (HIP kernel only)");
  const PngGeom g = png_geometry(warp_.H, warp_.W, rows_per_chunk);
  const int n = IMAGE_SHEETS * warp_.B;
  const size_t stride = (g.bound + 15) & ~(size_t)15, scratch = png_scratch_bytes(n, g);
  Stream& s = ctx_->s;
  stream_sync(s);                          // a replay in flight uses the buffers and the graph that are about to go
  graph_destroy(exec_); exec_ = nullptr; warmed_ = false;
  AllocScope mine(*ctx_, owned_);
  if (!png_streams_ || stride > png_stride_) png_streams_ = static_cast<uint8_t*>(ctx_->alloc((size_t)n * stride));
  if (!png_sizes_) png_sizes_ = static_cast<uint32_t*>(ctx_->alloc((size_t)n * sizeof(uint32_t)));
  if (!png_scratch_ || scratch > png_scratch_bytes_) { png_scratch_ = ctx_->alloc(scratch); png_scratch_bytes_ = scratch; }
  png_stride_ = std::max(png_stride_, stride);
  png_rows_ = rows_per_chunk;
}

void Pipeline::run(bool use_graph) {
  Stream& s = warp_.ctx->s;
  if (!use_graph) { enqueue(); return; }
  if (!exec_) {
    if (!warmed_) {             // first call: eager (kernel attributes, derived weight operands) -- results are this run's
      enqueue();
      warmed_ = true;
      if (!is_device_build()) return;
      stream_sync(s);
      // capture the identical sequence; nothing in it allocates, synchronises or depends on host state
      void* caller = s.handle;
      if (!cap_stream_) cap_stream_ = stream_create_current();
      s.handle = cap_stream_;
      try {
        graph_begin(s);
        try { enqueue(); } catch (...) { graph_abort(s); throw; }      // leave capture mode, keep the original error
        exec_ = graph_end(s);
      } catch (...) { s.handle = caller; throw; }
      s.handle = caller;
      return;
    }
    enqueue();                  // host simulator: no graphs
    return;
  }
  graph_launch(exec_, s);
}

}  // namespace swn
