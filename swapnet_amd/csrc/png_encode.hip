// swapnet_amd -- PNG encoding of saved images on the device (ops.h png_encode): what util.save_image (util/util.py:54-69) makes the host's
// zlib do per image -- row filtering and deflate -- as two launches over the bytes image_u8 left in HBM.  The encoder's body is
// png_chunk.h (filter choice, run-length tokens from a scan of the run starts, Huffman codes, bit packing, stored fallback, Adler-32);
// this unit holds the two kernels around it and their launcher.
//
// Shape: one workgroup of 256 threads per (image, chunk of R rows); the filtered chunk (R * (1 + 3W) bytes, 12.3 KB at W = 256) lives in
// LDS next to 19 KB of code tables, a thread owns ceil(bytes / 256) <= 128 consecutive positions.  The chunk kernel reads each image
// byte a few times (it is L2 traffic after the first) and writes one slot; the gather kernel copies the slots of an image back to back
// behind the zlib header and closes the stream with the combined Adler-32.  Fixed grids, no host read, no allocation: capturable.
#include "hip_util.h"
#include "png_chunk.h"

namespace swn {
namespace {

struct DevX {
  int tid;
  __device__ void sync() { __syncthreads(); }
};

struct POp {
  const uint8_t* img; uint8_t* slots; uint32_t* chunk_sizes; uint32_t* adler; uint8_t* streams; uint32_t* sizes;
  size_t image_bytes, slot, stream_stride;
  int H, W, R, chunks, chunk_bytes, last_bytes;
};

__global__ __launch_bounds__(PNG_THREADS) void png_chunk_kernel(const POp p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t png_filtered[];
  __shared__ PngShared sm;
  const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
  PngChunkArgs a;
  a.img = p.img + (size_t)b * p.image_bytes; a.H = p.H; a.W = p.W; a.R = p.R; a.chunk = chunk; a.last = chunk == p.chunks - 1;
  a.slot = reinterpret_cast<uint32_t*>(p.slots + (size_t)blockIdx.x * p.slot);
  a.size = p.chunk_sizes + blockIdx.x;
  a.adler = p.adler + 2 * (size_t)blockIdx.x;
  DevX x{(int)threadIdx.x};
  png_chunk_encode(x, sm, png_filtered, a);
}

constexpr int GATHER_THREADS = 1024;       // one workgroup copies a whole image: as many loads in flight as a workgroup can have

__global__ __launch_bounds__(GATHER_THREADS) void png_gather_kernel(const POp p) {
  const size_t b = blockIdx.x;
  PngGatherArgs g;
  g.chunks = p.chunks; g.slot_stride = p.slot; g.slots = p.slots + b * p.chunks * p.slot; g.sizes = p.chunk_sizes + b * p.chunks;
  g.adler = p.adler + 2 * b * p.chunks; g.chunk_bytes = p.chunk_bytes; g.last_bytes = p.last_bytes;
  g.stream = p.streams + b * p.stream_stride; g.size = p.sizes + b;
  DevX x{(int)threadIdx.x};
  png_gather<GATHER_THREADS>(x, g);
}

}  // namespace

void png_encode(Stream& s, const PngEncodeArgs& a) {
  if (!a.img || !a.scratch || !a.streams || !a.sizes) throw Error(1, "png_encode: NULL argument");
  if (a.n < 1) throw Error(1, "png_encode: empty batch");
  const PngGeom g = png_geometry(a.h, a.w, a.rows_per_chunk);
  if (a.stream_stride < g.bound)
    throw Error(1, "png_encode: stream_stride " + std::to_string(a.stream_stride) + " is below the bound " + std::to_string(g.bound));
  if ((uintptr_t)a.scratch & 3) throw Error(1, "png_encode: the scratch must be 4-byte aligned");
  if ((size_t)a.n * g.chunks > 0x7fffffffull) throw Error(1, "png_encode: batch too large for one launch");
  const size_t nchunks = (size_t)a.n * g.chunks;
  POp p{};
  p.img = a.img; p.slots = static_cast<uint8_t*>(a.scratch);
  p.chunk_sizes = reinterpret_cast<uint32_t*>(p.slots + nchunks * g.slot);
  p.adler = p.chunk_sizes + nchunks;
  p.streams = a.streams; p.sizes = a.sizes;
  p.image_bytes = (size_t)a.h * a.w * 3; p.slot = g.slot; p.stream_stride = a.stream_stride;
  p.H = a.h; p.W = a.w; p.R = g.R; p.chunks = g.chunks; p.chunk_bytes = g.chunk_bytes; p.last_bytes = g.last_bytes;
  const size_t lds = ((size_t)g.chunk_bytes + 15) & ~(size_t)15;         // <= 32 KB, next to the static tables: under the 64 KB default
  hipLaunchKernelGGL(png_chunk_kernel, dim3((unsigned)nchunks), dim3(PNG_THREADS), lds, hs(s), p);
  check_launch("png_encode (chunks)");
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)a.n), dim3(GATHER_THREADS), 0, hs(s), p);
  check_launch("png_encode (gather)");
}

}  // namespace swn
