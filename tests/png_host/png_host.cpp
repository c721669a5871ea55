// The body of the PNG encoder (swapnet_amd/csrc/png_chunk.h) run as PNG_THREADS host threads around a barrier: the same text the HIP
// kernels of png_encode.hip compile, so the tests that need no GPU (tests/test_png_encode.py) check the algorithm, and a build with
// -fsanitize=address,undefined or -fsanitize=thread checks its indices and its barriers.  Not part of the library: a test program.
//
//   png_host H W rows_per_chunk N in.raw out.bin      in: N images (H,W,3) uint8;  out: per image uint32 size, uint32 bound, `bound`
//                                                     bytes (the stream, then the 0xA5 fill the encoder must not have touched)
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../swapnet_amd/csrc/png_chunk.h"

using namespace swn;

struct HostX {
  int tid;
  pthread_barrier_t* bar;
  void sync() { pthread_barrier_wait(bar); }
};

struct Job {
  int tid;
  pthread_barrier_t* bar;
  PngShared* sm;
  uint8_t* f;
  const PngChunkArgs* chunk;      // one of the two
  const PngGatherArgs* gather;
};

static void* run(void* p) {
  Job* j = static_cast<Job*>(p);
  HostX x{j->tid, j->bar};
  if (j->chunk) png_chunk_encode(x, *j->sm, j->f, *j->chunk);
  else png_gather<PNG_THREADS>(x, *j->gather);
  return nullptr;
}

static void workgroup(const PngChunkArgs* c, const PngGatherArgs* g, PngShared* sm, uint8_t* f) {
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, nullptr, PNG_THREADS);
  std::vector<Job> jobs(PNG_THREADS);
  std::vector<pthread_t> th(PNG_THREADS);
  for (int t = 0; t < PNG_THREADS; ++t) { jobs[t] = Job{t, &bar, sm, f, c, g}; pthread_create(&th[t], nullptr, run, &jobs[t]); }
  for (int t = 0; t < PNG_THREADS; ++t) pthread_join(th[t], nullptr);
  pthread_barrier_destroy(&bar);
}

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: png_host H W rows_per_chunk N in.raw out.bin\n"); return 2; }
  const int H = std::atoi(argv[1]), W = std::atoi(argv[2]), N = std::atoi(argv[4]);
  int R = std::atoi(argv[3]);
  const int stride = 1 + 3 * W;
  if (R == 0) { R = PNG_MAX_CHUNK / stride; if (R > 16) R = 16; if (R < 1) R = 1; }
  if (H < 1 || W < 1 || W > PNG_MAX_WIDTH || N < 1 || (size_t)R * stride > PNG_MAX_CHUNK) { std::fprintf(stderr, "refused\n"); return 3; }
  if (R > H) R = H;
  const int chunks = (H + R - 1) / R, last_rows = H - (chunks - 1) * R;
  const size_t image = (size_t)H * W * 3, slot = png_slot_stride((size_t)R * stride);
  const size_t bound = 2 + (size_t)(chunks - 1) * png_chunk_cap((size_t)R * stride) + png_chunk_cap((size_t)last_rows * stride) + 4;
  std::vector<uint8_t> img(image * N);
  FILE* in = std::fopen(argv[5], "rb");
  if (!in || std::fread(img.data(), 1, img.size(), in) != img.size()) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(in);
  FILE* out = std::fopen(argv[6], "wb");
  if (!out) return 2;
  // exactly the sizes the device buffers have, so that a sanitizer sees a write past any of them
  std::vector<uint8_t> f(((size_t)R * stride + 3) & ~(size_t)3);
  PngShared* sm = new PngShared;
  for (int n = 0; n < N; ++n) {
    std::vector<uint32_t> slots(slot / 4 * chunks, 0xdeadbeefu), sizes(chunks), adler(2 * chunks);
    for (int c = 0; c < chunks; ++c) {
      PngChunkArgs a{img.data() + image * n, H, W, R, c, c == chunks - 1, slots.data() + slot / 4 * c, &sizes[c], &adler[2 * c]};
      workgroup(&a, nullptr, sm, f.data());
    }
    std::vector<uint8_t> stream(bound, 0xA5);
    uint32_t size = 0;
    PngGatherArgs g{chunks, slot, reinterpret_cast<const uint8_t*>(slots.data()), sizes.data(), adler.data(), R * stride, last_rows * stride,
                    stream.data(), &size};
    workgroup(nullptr, &g, sm, f.data());
    const uint32_t b32 = (uint32_t)bound;
    std::fwrite(&size, 4, 1, out); std::fwrite(&b32, 4, 1, out); std::fwrite(stream.data(), 1, bound, out);
  }
  delete sm;
  std::fclose(out);
  return 0;
}
