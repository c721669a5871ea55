// swapnet_amd -- the body of the PNG encoder (ops.h png_encode): one workgroup of PNG_THREADS threads turns a chunk of consecutive image
// rows into a piece of a zlib stream (RFC 1950 / 1951, PNG specification section 9), a second one strings an image's pieces together.
//
// The body is written against a small execution context X { int tid; void sync(); } and two atomics, with no wave intrinsic, so that the
// SAME text runs as the HIP kernels of png_encode.hip (sync = __syncthreads) and, for the tests that need no GPU, as PNG_THREADS host
// threads around a barrier (tests/png_host/png_host.cpp, also the place where a host sanitizer sees every index this file computes).
//
// Every loop's trip count comes from the shape of the call or from a table size of the format (286, 19, 15): nothing iterates "until
// the data says stop".  Where a step runs a data-dependent number of times (the Huffman merges, the length-limit repair) the loop runs
// to its format bound and the step is predicated.
//
// A chunk of N = rows * (1 + 3W) <= 32768 filtered bytes, thread t owning the positions [t * per, (t + 1) * per), per = ceil(N / 256) <= 128:
//   1. filter: all five filter types per row, cost = sum of min(b, 256 - b), smallest wins, ties to the lower type; the row above the
//      chunk's first row is read from the image (zeros above the image);
//   2. runs: a position starts a run when its byte differs from the one before.  A thread keeps the run starts of its own positions as
//      a 128-bit mask; the last start before and the first start after its segment come from a prefix maximum / suffix minimum over the
//      threads.  With j = distance to the run start and r = distance to the run end, a position j >= 1 lies u = (j - 1) mod 258 bytes
//      into a match of L = min(258, r + u) bytes at distance 1: a match token at u = 0, nothing behind it, and literals where L < 3 (so
//      runs shorter than four bytes and tails of one or two bytes stay literals).  Tokens are recomputed from that, never stored;
//   3. codes: histogram, Huffman lengths by rank sort + two-queue merge, limited to 15 (7 for the code-length code) by the Kraft
//      repair, canonical codes; the code-length sequence uses the zero-run symbols 17 and 18 and trims through HLIT / HCLEN;
//   4. bits: per-thread bit counts, prefix sum, every thread ORs its tokens into the (zeroed) slot at its own bit offset;
//   5. stored block instead wherever the dynamic block would not be smaller; 6. the chunk's Adler-32 partial.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

namespace swn {

constexpr int PNG_THREADS = 256;
constexpr int PNG_MAX_CHUNK = 32768;        // bytes of a filtered chunk: one stored block, 128 positions per thread
constexpr int PNG_MAX_WIDTH = 2048;
constexpr uint32_t PNG_ADLER = 65521;

// capacity of a chunk's output slot: the stored form (5 bytes per block of at most 65535) plus the flush marker and slack
PNG_HD size_t png_chunk_cap(size_t n) { return n + 5 * ((n + 65534) / 65535) + 9; }
PNG_HD size_t png_slot_stride(size_t n) { return (png_chunk_cap(n) + 3) & ~(size_t)3; }      // slots are written as 32-bit words

template <class T>
PNG_HD void png_atomic_add(T* p, T v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // (only this workgroup touches what it adds to)
#else
  __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#endif
}
PNG_HD void png_atomic_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  __atomic_fetch_or(p, v, __ATOMIC_RELAXED);
#endif
}

struct PngShared {
  uint32_t freq[288];                       // literal / length histogram (286 symbols)
  uint32_t iw[288];                         // weights of the merged (internal) nodes, in creation order
  uint32_t sw[288];                         // weights of the used symbols, ascending
  uint16_t sorted[288], par_leaf[288], par_int[288], depth_int[288];
  uint16_t code[288];                       // canonical codes, bit-reversed: ready for LSB-first packing
  uint8_t len[288];
  uint8_t cl_in[288];                       // the code lengths to transmit: HLIT + 257 literal / length ones, then the distance one
  uint16_t cl_tok[320];                     // code-length tokens: symbol | extra << 8
  uint32_t cl_freq[19];
  uint16_t cl_code[19];
  uint8_t cl_len[19];
  uint32_t scan[PNG_THREADS], scan2[PNG_THREADS];
  uint32_t cost[PNG_THREADS][5];
  uint64_t adler_b[PNG_THREADS];
  uint32_t adler_a[PNG_THREADS];
  int num_codes[17], start[17], next_code[17];
  int nused, cl_ntok, nl, hclen, dist_used, stored;
  uint32_t hdr_bits, block_bits, size;
};

struct PngChunkArgs {
  const uint8_t* img;                       // this image: (H, W, 3)
  int H, W, R, chunk;                       // rows per chunk, this chunk's index
  int last;                                 // the image's last chunk: BFINAL
  uint32_t* slot;                           // png_slot_stride(R * (1 + 3W)) bytes, 4-byte aligned
  uint32_t* size;                           // bytes written to the slot
  uint32_t* adler;                          // (a, b) of the chunk's filtered bytes, from (1, 0)
};

PNG_HD int png_filter_byte(const uint8_t* img, int W, int y, int x, int type) {      // x = byte within the row, y = image row
  const size_t row = (size_t)y * W * 3;
  const int v = img[row + x];
  const int a = x >= 3 ? img[row + x - 3] : 0;
  const int b = y > 0 ? img[row - (size_t)W * 3 + x] : 0;
  const int c = (x >= 3 && y > 0) ? img[row - (size_t)W * 3 + x - 3] : 0;
  int pred = 0;
  if (type == 1) pred = a;
  else if (type == 2) pred = b;
  else if (type == 3) pred = (a + b) >> 1;
  else if (type == 4) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (v - pred) & 255;
}

// length 3 .. 258 -> (symbol - 257, number of extra bits, their value)
PNG_HD void png_length_code(int L, int* code, int* nextra, int* extra) {
  const int l = L - 3;
  if (L == 258) { *code = 28; *nextra = 0; *extra = 0; return; }
  if (l < 8) { *code = l; *nextra = 0; *extra = 0; return; }
  const int eb = (31 - __builtin_clz((unsigned)l)) - 2;
  *code = 4 * eb + 4 + ((l >> eb) & 3); *nextra = eb; *extra = l & ((1 << eb) - 1);
}
PNG_HD int png_length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

PNG_HD uint32_t png_reverse_bits(uint32_t c, int n) {
  uint32_t r = 0;
  for (int i = 0; i < 15; ++i) if (i < n) r |= ((c >> i) & 1u) << (n - 1 - i);
  return r;
}

// Huffman code of `n` <= 286 symbols with lengths <= maxlen: len[] (0 = unused) and bit-reversed canonical code[].  All threads call.
template <class X>
PNG_HD void png_build_code(X& x, PngShared& sm, const uint32_t* freq, int n, int maxlen, uint8_t* len, uint16_t* code) {
  const int tid = x.tid;
  if (tid == 0) sm.nused = 0;
  x.sync();
  for (int s = tid; s < n; s += PNG_THREADS) {                // rank sort by (frequency, symbol), unused symbols left out
    len[s] = 0;
    const uint32_t f = freq[s];
    if (f) {
      int rank = 0;
      for (int q = 0; q < n; ++q) { const uint32_t g = freq[q]; rank += (g != 0 && (g < f || (g == f && q < s))) ? 1 : 0; }
      sm.sorted[rank] = (uint16_t)s; sm.sw[rank] = f;
      png_atomic_add(&sm.nused, 1);
    }
  }
  x.sync();
  if (tid == 0) {
    const int m = sm.nused;
    for (int l = 0; l <= 16; ++l) sm.num_codes[l] = 0;
    if (m == 1) sm.num_codes[1] = 1;                          // a code of one symbol still gets one bit
    if (m >= 2) {
      int li = 0, ii = 0;                                     // heads of the leaf queue and of the merged-node queue,
      uint32_t lw = sm.sw[0], nw = 0;                         // their weights kept in registers: one LDS round trip per pick
      for (int k = 0; k < n - 1; ++k) {
        if (k < m - 1) {
          uint32_t w = 0;
          for (int pick = 0; pick < 2; ++pick) {
            const bool leaf_ok = li < m, int_ok = ii < k;
            if (leaf_ok && (!int_ok || lw <= nw)) { w += lw; sm.par_leaf[li] = (uint16_t)k; ++li; lw = sm.sw[li]; }
            else { w += nw; sm.par_int[ii] = (uint16_t)k; ++ii; nw = sm.iw[ii]; }
          }
          sm.iw[k] = w;
          if (ii == k) nw = w;                                // (the queue was empty: the new node is its head)
        }
      }
      for (int k = n - 2; k >= 0; --k)                        // a node's parent was created after it: depths from the root down
        if (k <= m - 2) sm.depth_int[k] = k == m - 2 ? 0 : (uint16_t)(sm.depth_int[sm.par_int[k]] + 1);
    }
  }
  x.sync();
  for (int i = tid; i < n; i += PNG_THREADS)                  // leaf depths, cut to maxlen, counted per length
    if (sm.nused >= 2 && i < sm.nused) { const int d = sm.depth_int[sm.par_leaf[i]] + 1; png_atomic_add(&sm.num_codes[d < maxlen ? d : maxlen], 1); }
  x.sync();
  if (tid == 0) {
    const int m = sm.nused;
    if (m >= 2) {
      // lengths cut to maxlen oversubscribe the code: trade one maxlen code and one shorter code for two of the next length, once
      // per unit of excess (the excess is below the number of cut codes, hence below n)
      uint32_t total = 0;
      for (int l = maxlen; l >= 1; --l) total += (uint32_t)sm.num_codes[l] << (maxlen - l);
      for (int it = 0; it < n; ++it) {
        if (total != (1u << maxlen)) {
          sm.num_codes[maxlen]--;
          bool done = false;
          for (int l = maxlen - 1; l >= 1; --l)
            if (!done && sm.num_codes[l]) { sm.num_codes[l]--; sm.num_codes[l + 1] += 2; done = true; }
          total--;
        }
      }
    }
    int acc = 0;                                              // ascending frequency: the longest codes come first
    for (int l = maxlen; l >= 1; --l) { sm.start[l] = acc; acc += sm.num_codes[l]; }
    int c = 0;
    sm.next_code[0] = 0;
    for (int l = 1; l <= maxlen; ++l) { c = (c + sm.num_codes[l - 1]) << 1; sm.next_code[l] = c; }
  }
  x.sync();
  for (int i = tid; i < n; i += PNG_THREADS) {
    if (i < sm.nused) {
      int L = 0;
      for (int l = 1; l <= 15; ++l) if (l <= maxlen && i >= sm.start[l] && i < sm.start[l] + sm.num_codes[l]) L = l;
      len[sm.sorted[i]] = (uint8_t)L;
    }
  }
  x.sync();
  for (int s = tid; s < n; s += PNG_THREADS) {                // canonical: within a length, codes ascend with the symbol
    const int L = len[s];
    uint32_t c = 0;
    if (L) {
      c = (uint32_t)sm.next_code[L];
      for (int q = 0; q < n; ++q) c += (q < s && len[q] == L) ? 1u : 0u;
    }
    code[s] = (uint16_t)png_reverse_bits(c, L);
  }
  x.sync();
}

// the run starts a thread knows: those of its own positions, the last one before them and the first one after them
struct PngRuns {
  uint64_t lo, hi;
  int base, per, N, prev_start, next_start;
};
PNG_HD int png_next_start(const PngRuns& r, int l) {           // first run start behind local position l
  if (l < 63) { const uint64_t m = r.lo & (~0ull << (l + 1)); if (m) return r.base + __builtin_ctzll(m); }
  if (l < 127) { const uint64_t h = l < 64 ? r.hi : (r.hi & (~0ull << (l - 63))); if (h) return r.base + 64 + __builtin_ctzll(h); }
  return r.next_start;
}
// calls lit(byte) / match(length) for the tokens that START at this thread's positions, in order
template <class Lit, class Match>
PNG_HD void png_walk(const PngRuns& r, const uint8_t* f, Lit&& lit, Match&& match) {
  int s = r.prev_start;
  for (int l = 0; l < r.per; ++l) {
    const int i = r.base + l;
    if (i < r.N) {
      if ((l < 64 ? (r.lo >> l) : (r.hi >> (l - 64))) & 1) s = i;
      const int j = i - s;
      if (j == 0) { lit(f[i]); continue; }
      const int u = (j - 1) % 258;
      int L = png_next_start(r, l) - i + u;
      if (L > 258) L = 258;
      if (L < 3) lit(f[i]);
      else if (u == 0) match(L);
    }
  }
}

struct PngBits {                            // LSB-first bit writer into zeroed 32-bit words that other threads OR into as well
  uint32_t* w; uint64_t acc; int fill; uint32_t word;
  PNG_HD PngBits(uint32_t* base, uint32_t bit) : w(base), acc(0), fill((int)(bit & 31)), word(bit >> 5) {}
  PNG_HD void put(uint32_t v, int n) {      // n <= 16
    acc |= (uint64_t)v << fill; fill += n;
    if (fill >= 32) { png_atomic_or(w + word, (uint32_t)acc); acc >>= 32; fill -= 32; ++word; }
  }
  PNG_HD void flush() { if (fill > 0) png_atomic_or(w + word, (uint32_t)acc); fill = 0; acc = 0; }
};

// f: N bytes (rounded up to 4) of workgroup memory for the filtered chunk
template <class X>
PNG_HD void png_chunk_encode(X& x, PngShared& sm, uint8_t* f, const PngChunkArgs& a) {
  const int tid = x.tid;
  const int rowbytes = 3 * a.W, stride = rowbytes + 1;
  const int y0 = a.chunk * a.R;
  const int rows = a.H - y0 < a.R ? a.H - y0 : a.R;
  const int N = rows * stride;
  const int slot_words = (int)(png_slot_stride((size_t)a.R * stride) >> 2);
  for (int i = tid; i < slot_words; i += PNG_THREADS) a.slot[i] = 0u;

  // ---- 1. filter choice: P threads per row, rpp rows per pass ----
  const int P = rows >= PNG_THREADS ? 1 : PNG_THREADS / rows, rpp = PNG_THREADS / P;
  const int seg = (rowbytes + P - 1) / P;
  for (int r0 = 0; r0 < rows; r0 += rpp) {
    const int row = r0 + tid / P, part = tid % P;
    const bool mine = tid / P < rpp && row < rows;
    if (mine) {
      uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
      const int x1 = (part + 1) * seg < rowbytes ? (part + 1) * seg : rowbytes;
      for (int xx = part * seg; xx < x1; ++xx)
        for (int t = 0; t < 5; ++t) { const int v = png_filter_byte(a.img, a.W, y0 + row, xx, t); c[t] += (uint32_t)(v < 256 - v ? v : 256 - v); }
      for (int t = 0; t < 5; ++t) sm.cost[tid][t] = c[t];
    }
    x.sync();
    if (mine && part == 0) {
      uint32_t best = 0xffffffffu; int type = 0;
      for (int t = 0; t < 5; ++t) {
        uint32_t c = 0;
        for (int p = 0; p < P; ++p) c += sm.cost[tid + p][t];
        if (c < best) { best = c; type = t; }                 // strict: ties go to the lower type
      }
      f[row * stride] = (uint8_t)type;
    }
    x.sync();
  }
  for (int i = tid; i < N; i += PNG_THREADS) {
    const int row = i / stride, xx = i - row * stride;
    if (xx > 0) f[i] = (uint8_t)png_filter_byte(a.img, a.W, y0 + row, xx - 1, f[row * stride]);
  }
  x.sync();

  // ---- 2. run starts of this thread's positions; 6. Adler-32 partial sums ----
  PngRuns r;
  r.per = (N + PNG_THREADS - 1) / PNG_THREADS; r.base = tid * r.per; r.N = N; r.lo = 0; r.hi = 0;
  {
    uint32_t sa = 0; uint64_t sb = 0;
    for (int l = 0; l < r.per; ++l) {
      const int i = r.base + l;
      if (i < N) {
        const uint32_t d = f[i];
        if (i == 0 || f[i - 1] != d) { if (l < 64) r.lo |= 1ull << l; else r.hi |= 1ull << (l - 64); }
        sa += d; sb += (uint64_t)(N - i) * d;
      }
    }
    sm.adler_a[tid] = sa; sm.adler_b[tid] = sb;
    const int last = r.hi ? r.base + 127 - __builtin_clzll(r.hi) : (r.lo ? r.base + 63 - __builtin_clzll(r.lo) : -1);
    const int first = r.lo ? r.base + __builtin_ctzll(r.lo) : (r.hi ? r.base + 64 + __builtin_ctzll(r.hi) : N);
    sm.scan[tid] = (uint32_t)(last + 1); sm.scan2[tid] = (uint32_t)first;
  }
  for (int s = tid; s < 288; s += PNG_THREADS) sm.freq[s] = 0u;
  x.sync();
  {
    uint32_t prev = 0, next = (uint32_t)N;
    for (int q = 0; q < PNG_THREADS; ++q) {
      if (q < tid && sm.scan[q] > prev) prev = sm.scan[q];
      if (q > tid && sm.scan2[q] < next) next = sm.scan2[q];
    }
    r.prev_start = (int)prev - 1;           // (thread 0 has none: position 0 starts a run)
    r.next_start = (int)next;
  }
  if (tid == 0) {
    uint64_t sa = 1, sb = (uint64_t)N;
    for (int q = 0; q < PNG_THREADS; ++q) { sa += sm.adler_a[q]; sb += sm.adler_b[q]; }
    a.adler[0] = (uint32_t)(sa % PNG_ADLER); a.adler[1] = (uint32_t)(sb % PNG_ADLER);
  }

  // ---- 3. histogram and codes ----
  png_walk(r, f,
           [&](int b) { png_atomic_add(&sm.freq[b], 1u); },
           [&](int L) { int c, ne, ev; png_length_code(L, &c, &ne, &ev); png_atomic_add(&sm.freq[257 + c], 1u); });
  if (tid == 0) png_atomic_add(&sm.freq[256], 1u);
  x.sync();
  png_build_code(x, sm, sm.freq, 286, 15, sm.len, sm.code);
  int nl = 257; uint32_t nmatch = 0;        // (every thread for itself: 29 broadcast reads)
  for (int s = 257; s < 286; ++s) if (sm.freq[s]) { nl = s + 1; nmatch += sm.freq[s]; }
  for (int i = tid; i < nl; i += PNG_THREADS) sm.cl_in[i] = sm.len[i];
  if (tid < 19) sm.cl_freq[tid] = 0u;
  if (tid == 0) {
    sm.nl = nl; sm.dist_used = nmatch ? 1 : 0;
    sm.cl_in[nl] = (uint8_t)sm.dist_used;   // one distance code (distance 1) of one bit, or none at all
    sm.hdr_bits = 0; sm.block_bits = 0;
  }
  x.sync();
  if (tid == 0) {
    int nt = 0, z = 0;
    auto tok = [&](int sym, int extra) { sm.cl_tok[nt++] = (uint16_t)(sym | (extra << 8)); sm.cl_freq[sym]++; };
    for (int i = 0; i <= 287; ++i) {
      if (i <= nl + 1) {                    // i == nl + 1: behind the end, flushes the zeros
        const int v = i <= nl ? sm.cl_in[i] : 1;
        if (v == 0) {
          if (++z == 138) { tok(18, 138 - 11); z = 0; }
        } else {
          if (z >= 11) tok(18, z - 11);
          else if (z >= 3) tok(17, z - 3);
          else { if (z >= 1) tok(0, 0); if (z >= 2) tok(0, 0); }
          z = 0;
          if (i <= nl) tok(v, 0);
        }
      }
    }
    sm.cl_ntok = nt;
  }
  png_build_code(x, sm, sm.cl_freq, 19, 7, sm.cl_len, sm.cl_code);
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (int i = tid; i < 320; i += PNG_THREADS)                 // bits of the code-length tokens, bits of the block's symbols
    if (i < sm.cl_ntok) { const int sym = sm.cl_tok[i] & 255; png_atomic_add(&sm.hdr_bits, sm.cl_len[sym] + (sym == 17 ? 3u : sym == 18 ? 7u : 0u)); }
  for (int s = tid; s < 286; s += PNG_THREADS)
    if (sm.freq[s]) png_atomic_add(&sm.block_bits, sm.freq[s] * (uint32_t)(sm.len[s] + (s > 256 ? png_length_extra_bits(s) + 1 : 0)));
  x.sync();
  if (tid == 0) {
    int hclen = 4;
    for (int i = 4; i < 19; ++i) if (sm.cl_len[order[i]]) hclen = i + 1;
    sm.hclen = hclen;
    const uint32_t hdr = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen + sm.hdr_bits, body = sm.block_bits;
    sm.hdr_bits = hdr; sm.block_bits = hdr + body;
    const uint32_t dyn = a.last ? (hdr + body + 7) / 8 : (hdr + body + 3 + 7) / 8 + 4;
    sm.stored = dyn >= (uint32_t)N + 5 ? 1 : 0;
    sm.size = sm.stored ? (uint32_t)N + 5 : dyn;
    *a.size = sm.size;
  }
  x.sync();

  // ---- 5. stored block ----
  if (sm.stored) {
    uint8_t* out = reinterpret_cast<uint8_t*>(a.slot);
    if (tid == 0) {
      out[0] = (uint8_t)(a.last ? 1 : 0);
      out[1] = (uint8_t)(N & 255); out[2] = (uint8_t)(N >> 8); out[3] = (uint8_t)(~N & 255); out[4] = (uint8_t)((~N >> 8) & 255);
    }
    for (int i = tid; i < N; i += PNG_THREADS) out[5 + i] = f[i];
    return;
  }

  // ---- 4. bit offsets and packing ----
  {
    uint32_t bits = 0;
    png_walk(r, f,
             [&](int b) { bits += sm.len[b]; },
             [&](int L) { int c, ne, ev; png_length_code(L, &c, &ne, &ev); bits += sm.len[257 + c] + (uint32_t)ne + 1u; });
    sm.scan[tid] = bits;
  }
  x.sync();
  uint32_t at = sm.hdr_bits;
  for (int q = 0; q < PNG_THREADS; ++q) if (q < tid) at += sm.scan[q];
  {
    PngBits w(a.slot, at);
    png_walk(r, f,
             [&](int b) { w.put(sm.code[b], sm.len[b]); },
             [&](int L) {
               int c, ne, ev; png_length_code(L, &c, &ne, &ev);
               w.put(sm.code[257 + c], sm.len[257 + c]);
               if (ne) w.put((uint32_t)ev, ne);
               w.put(0u, 1);                                   // distance symbol 0 (distance 1), the one-bit code 0
             });
    w.flush();
  }
  if (tid == 0) {
    PngBits w(a.slot, 0);
    w.put(a.last ? 1u : 0u, 1); w.put(2u, 2);                  // BFINAL, BTYPE = 10: dynamic Huffman
    w.put((uint32_t)(sm.nl - 257), 5); w.put(0u, 5); w.put((uint32_t)(sm.hclen - 4), 4);
    for (int i = 0; i < 19; ++i) if (i < sm.hclen) w.put(sm.cl_len[order[i]], 3);
    for (int i = 0; i < 320; ++i) {
      if (i < sm.cl_ntok) {
        const int sym = sm.cl_tok[i] & 255, extra = sm.cl_tok[i] >> 8;
        w.put(sm.cl_code[sym], sm.cl_len[sym]);
        if (sym == 17) w.put((uint32_t)extra, 3);
        if (sym == 18) w.put((uint32_t)extra, 7);
      }
    }
    w.flush();
    PngBits e(a.slot, sm.block_bits - sm.len[256]);
    e.put(sm.code[256], sm.len[256]);
    if (!a.last) {                                             // empty stored block: the next chunk starts on a byte
      e.put(0u, 3);
      e.put(0u, (8 - (e.fill & 7)) & 7);
      e.put(0u, 16); e.put(0xffffu, 16);
    }
    e.flush();
  }
}

struct PngGatherArgs {
  int chunks;
  size_t slot_stride;                       // bytes between an image's chunk slots
  const uint8_t* slots;                     // this image's first slot
  const uint32_t* sizes;                    // this image's chunk sizes
  const uint32_t* adler;                    // (a, b) per chunk
  int chunk_bytes, last_bytes;              // filtered bytes of a full chunk / of the last chunk
  uint8_t* stream;                          // 2 + sum of the slots' capacities + 4 bytes at least
  uint32_t* size;
};

// NT threads.  The slots are word-aligned, the place of a chunk in the stream is not: 32-bit loads, byte stores.
template <int NT, class X>
PNG_HD void png_gather(X& x, const PngGatherArgs& g) {
  const int tid = x.tid;
  const uint32_t cap = (uint32_t)png_chunk_cap((size_t)g.chunk_bytes);
  const uint32_t words = (uint32_t)(g.slot_stride >> 2);
  if (tid == 0) { g.stream[0] = 0x78; g.stream[1] = 0x01; }   // deflate, 32K window, no dictionary, fastest
  size_t off = 2;                           // every thread keeps the running sum of the sizes: they are uniform
  for (int c = 0; c < g.chunks; ++c) {
    const uint32_t sz = g.sizes[c] < cap ? g.sizes[c] : cap;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(g.slots + (size_t)c * g.slot_stride);
    uint8_t* dst = g.stream + off;
    for (uint32_t i = (uint32_t)tid; i < words; i += NT) {
      const uint32_t v = src[i], b = 4 * i;
      if (b < sz) dst[b] = (uint8_t)v;
      if (b + 1 < sz) dst[b + 1] = (uint8_t)(v >> 8);
      if (b + 2 < sz) dst[b + 2] = (uint8_t)(v >> 16);
      if (b + 3 < sz) dst[b + 3] = (uint8_t)(v >> 24);
    }
    off += sz;
  }
  if (tid == 0) {
    uint64_t a = 1, b = 0;
    for (int c = 0; c < g.chunks; ++c) {
      const uint64_t a2 = g.adler[2 * c], b2 = g.adler[2 * c + 1], len2 = (uint64_t)(c == g.chunks - 1 ? g.last_bytes : g.chunk_bytes);
      b = (b + b2 + len2 % PNG_ADLER * ((a + PNG_ADLER - 1) % PNG_ADLER)) % PNG_ADLER;
      a = (a + a2 + PNG_ADLER - 1) % PNG_ADLER;
    }
    const uint32_t ad = (uint32_t)((b << 16) | a);
    g.stream[off] = (uint8_t)(ad >> 24); g.stream[off + 1] = (uint8_t)(ad >> 16); g.stream[off + 2] = (uint8_t)(ad >> 8); g.stream[off + 3] = (uint8_t)ad;
    *g.size = (uint32_t)(off + 4);
  }
}

}  // namespace swn
