// Host check of the filter's host bookkeeping: FeatureTable (csrc/ekf_feature_table.hpp) replays the operation
// sequences of tools/filter_host_check.py and is compared with the Python model after every operation, bit for bit;
// ReadBack, InputRing and LaunchProfiler (csrc/ekf_buffers.hpp) run against the stand-in HIP calls below.  A program of its
// own, built with -fsanitize=address,undefined by tests/test_host_checks.py: no device, no HIP library, nothing loaded into Python.
// Usage: filter_host_check CASE.bin ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_buffers.hpp"
#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_feature_table.hpp"

// ---- stand-ins for the HIP calls ekf_buffers.hpp makes -------------------------------------------------------------------
// Memory is the host's (the sanitizer watches every block).  A copy is only QUEUED by the copy call; it is carried out by
// the stream synchronisation, or by the synchronisation of an event recorded behind it -- so a piece handed to its place
// early, a pinned slot rewritten while its copy is in flight or a copy out of a buffer that has moved shows.
struct Copy { char* dst; size_t dpitch; const char* src; size_t spitch, width, rows; };
struct ihipEvent_t { size_t mark; };
static std::vector<Copy> g_queue;
static size_t g_done = 0;                      // copies of g_queue carried out so far
static int g_copy_calls = 0, g_fail_copy_at = -1, g_stream_syncs = 0, g_event_waits = 0, g_events_live = 0, g_events_made = 0;
static int g_allocs_live = 0;
static bool g_fail_sync = false, g_fail_alloc = false;
static hipEvent_t g_last_waited = nullptr;
static std::vector<hipEvent_t> g_created;     // every event ever made, in order (compared by address only)

static void run_copies(size_t upto) {
  for (; g_done < upto; ++g_done) {
    const Copy& c = g_queue[g_done];
    for (size_t r = 0; r < c.rows; ++r) memcpy(c.dst + r * c.dpitch, c.src + r * c.spitch, c.width);
  }
  if (g_done == g_queue.size()) { g_queue.clear(); g_done = 0; }
}
static hipError_t queue_copy(const Copy& c) {
  if (g_copy_calls++ == g_fail_copy_at) return hipErrorInvalidValue;
  g_queue.push_back(c);
  return hipSuccess;
}
static hipError_t host_alloc(void** p, size_t bytes) {
  if (g_fail_alloc) { g_fail_alloc = false; *p = nullptr; return hipErrorOutOfMemory; }
  *p = malloc(bytes);
  ++g_allocs_live;
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
extern "C" {
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return host_alloc(p, bytes); }
hipError_t hipHostFree(void* p) { free(p); --g_allocs_live; return hipSuccess; }
hipError_t hipMalloc(void** p, size_t bytes) { return host_alloc(p, bytes); }
hipError_t hipFree(void* p) { free(p); --g_allocs_live; return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  return queue_copy({static_cast<char*>(dst), 0, static_cast<const char*>(src), 0, bytes, 1});
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind,
                            hipStream_t) {
  return queue_copy({static_cast<char*>(dst), dpitch, static_cast<const char*>(src), spitch, width, height});
}
hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_stream_syncs;
  if (g_fail_sync) { g_fail_sync = false; return hipErrorUnknown; }
  run_copies(g_queue.size());
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { *e = new ihipEvent_t{0}; g_created.push_back(*e); ++g_events_live; ++g_events_made; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { delete e; --g_events_live; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->mark = g_queue.size(); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) {
  ++g_event_waits;
  g_last_waited = e;
  run_copies(e->mark < g_queue.size() ? e->mark : g_queue.size());   // (a queue that was drained since holds nothing of this event's)
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 1.5f; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
}

static int g_failed = 0;
#define CHECK(cond) \
  do { if (!(cond)) { printf("%s:%d: CHECK(%s) DIFFERS\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

// ---- the feature table against the Python model ----------------------------------------------------------------------------
struct Words {
  std::vector<int> w;
  size_t at = 0;
  bool ok = true;
  int next() { if (at >= w.size()) { ok = false; return 0; } return w[at++]; }
  std::vector<int> take(int count) { std::vector<int> v; for (int i = 0; i < count; ++i) v.push_back(next()); return v; }
};
static float as_float(int bits) { float f; memcpy(&f, &bits, sizeof(f)); return f; }
static int as_bits(float f) { int b; memcpy(&b, &f, sizeof(b)); return b; }

static bool table_equals(const ekf::FeatureTable& ft, Words& in) {
  const int N = in.next(), next_real = in.next();
  const std::vector<int> pos = in.take(N), coding = in.take(N), real = in.take(N), nfind = in.take(N), ntot = in.take(N),
                         cen = in.take(2 * N), inn = in.take(N), rem = in.take(N);
  const ekf::FeatureTable::Columns& c = ft.columns();
  bool same = ft.size() == N && ft.next_real_index() == next_real;
  // every column has the table's length: the invariant no caller keeps by hand any more
  same = same && (int)c.pos.size() == N && (int)c.coding.size() == N && (int)c.real_index.size() == N && (int)c.n_find.size() == N &&
         (int)c.n_tot.size() == N && (int)c.center.size() == 2 * N && (int)c.in_innovation.size() == N && (int)c.remove_flag.size() == N;
  for (int i = 0; same && i < N; ++i)
    same = ft.pos(i) == pos[i] && ft.coding(i) == coding[i] && ft.real_index(i) == real[i] && ft.n_find(i) == nfind[i] &&
           ft.n_tot(i) == ntot[i] && as_bits(ft.center(i)[0]) == cen[2 * i] && as_bits(ft.center(i)[1]) == cen[2 * i + 1] &&
           (int)ft.in_innovation(i) == inn[i] && (int)ft.remove_flag(i) == rem[i] && c.pos[i] == pos[i] && c.coding[i] == coding[i] &&
           c.real_index[i] == real[i];
  return same;
}

static void replay(const char* path) {
  Words in;
  if (FILE* fh = fopen(path, "rb")) {
    int v;
    while (fread(&v, sizeof(v), 1, fh) == 1) in.w.push_back(v);
    fclose(fh);
  }
  const int camera_dim = in.next(), ops = in.next();
  ekf::FeatureTable ft;
  int bad = 0, compactions = 0;
  for (int k = 0; k < ops && in.ok; ++k) {
    const int op = in.next();
    std::vector<int> msrc, mconv;
    if (op == 1) {
      const int row = in.next(), u = in.next(), v = in.next();
      ft.add(row, as_float(u), as_float(v));
    } else if (op == 2) {
      const int N = ft.size();
      const std::vector<int> rm_i = in.take(N), cv_i = in.take(N);
      const std::vector<char> rm(rm_i.begin(), rm_i.end()), cv(cv_i.begin(), cv_i.end());
      ekf::FeatureTable::Compaction next = ft.compacted(rm, cv, camera_dim);
      ft.adopt(std::move(next.cols));
      msrc = next.msrc; mconv = next.mconv;
      ++compactions;
    } else if (op == 3) {
      const std::vector<int> b_i = in.take(ft.size());
      ft.fold_track(std::vector<unsigned char>(b_i.begin(), b_i.end()));
    } else if (op == 4) {
      const int i = in.next(), ri = in.next(), nf = in.next();
      ft.set_meta(i, ri, nf);
    } else if (op == 5) {
      const int i = in.next(), nt = in.next(), inn = in.next(), has = in.next();
      const float cen[2] = {as_float(in.next()), as_float(in.next())};
      const int rem = in.next();
      ft.set_track(i, nt, inn, has ? cen : nullptr, rem);
    } else if (op == 6) {
      const int i = in.next(), found = in.next(), u = in.next(), v = in.next();
      ft.searched(i, found != 0, as_float(u), as_float(v));
    } else if (op == 7) {
      ft.count_found(in.next());
    } else if (op == 8) {
      ft.flag_removal(in.next());
    } else {
      in.ok = false;
    }
    bool same = table_equals(ft, in);
    if (op == 2) {
      const int n_new = in.next();
      same = same && in.take(n_new) == msrc && in.take(n_new) == mconv && (int)msrc.size() == n_new;
    }
    if (!same) { printf("%s: operation %d (kind %d) DIFFERS\n", path, k, op); ++bad; }
  }
  if (!in.ok || in.at != in.w.size()) { printf("%s: case file and replay are out of step DIFFERS\n", path); ++bad; }
  const std::string p(path);
  printf("%s: %d operations, %d compactions, %d features left: %s\n", p.substr(p.find_last_of('/') + 1).c_str(), ops, compactions,
         ft.size(), bad ? "DIFFERS" : "equal");
  g_failed += bad;
}

// ---- the read-back queue ----------------------------------------------------------------------------------------------------
static std::vector<char> pattern(size_t bytes, int seed) {
  std::vector<char> v(bytes);
  for (size_t i = 0; i < bytes; ++i) v[i] = (char)((i * 31 + seed * 7 + (i >> 8)) & 0xff);
  return v;
}
static bool all_are(const std::vector<char>& v, char c) { for (char x : v) if (x != c) return false; return true; }

static void check_readback() {
  hipStream_t st = nullptr;
  {
    ekf::ReadBack rb;                                         // first use: 64 KiB; the piece arrives at finish(), not before
    const std::vector<char> src = pattern(100, 1);
    std::vector<char> dst(100, (char)0xEE);
    CHECK(rb.capacity() == 0 && rb.add(dst.data(), src.data(), 100, st) == hipSuccess);
    CHECK(rb.capacity() == 65536 && rb.pending() == 1 && rb.offset() == 112 && all_are(dst, (char)0xEE));
    const int syncs = g_stream_syncs;
    CHECK(rb.finish(st) == hipSuccess && g_stream_syncs == syncs + 1 && dst == src && rb.pending() == 0 && rb.offset() == 0);

    // the edge: 65472 + 64 bytes of slack fill the buffer; the next piece finds no room, the first is delivered mid-batch
    const std::vector<char> big = pattern(65472, 2), small = pattern(16, 3);
    std::vector<char> dbig(65472, (char)0xEE), dsmall(16, (char)0xEE);
    CHECK(rb.add(dbig.data(), big.data(), 65472, st) == hipSuccess && rb.capacity() == 65536 && rb.offset() == 65472);
    CHECK(all_are(dbig, (char)0xEE) && g_stream_syncs == syncs + 1);
    CHECK(rb.add(dsmall.data(), small.data(), 16, st) == hipSuccess);
    CHECK(g_stream_syncs == syncs + 2 && dbig == big && all_are(dsmall, (char)0xEE));          // delivered; the new piece still queued
    CHECK(rb.capacity() == 65536 && rb.pending() == 1 && rb.offset() == 16);                   // ... at offset 0 of the same buffer
    CHECK(rb.finish(st) == hipSuccess && dsmall == small);

    // larger than the buffer, nothing pending: it grows to twice the piece and its slack, with no synchronisation
    const std::vector<char> huge = pattern(200000, 4);
    std::vector<char> dhuge(200000, (char)0xEE);
    CHECK(rb.add(dhuge.data(), huge.data(), 200000, st) == hipSuccess && rb.capacity() == 2 * (200000 + 64));
    CHECK(g_stream_syncs == syncs + 3 && rb.finish(st) == hipSuccess && dhuge == huge);
    // ... and with a piece pending: that one is delivered out of the old buffer before the buffer moves
    const std::vector<char> huger = pattern(500000, 5);
    std::vector<char> dhuger(500000, (char)0xEE);
    std::fill(dsmall.begin(), dsmall.end(), (char)0xEE);
    CHECK(rb.add(dsmall.data(), small.data(), 16, st) == hipSuccess && rb.add(dhuger.data(), huger.data(), 500000, st) == hipSuccess);
    CHECK(dsmall == small && rb.capacity() == 2 * (500000 + 64) && rb.pending() == 1 && all_are(dhuger, (char)0xEE));
    CHECK(rb.finish(st) == hipSuccess && dhuger == huger);
  }
  {
    ekf::ReadBack rb;                                         // failures: nothing stays queued, the next batch starts at offset 0
    const std::vector<char> a = pattern(48, 6), b = pattern(40, 7);
    std::vector<char> da(48, (char)0xEE), db(40, (char)0xEE);
    CHECK(rb.add(da.data(), a.data(), 48, st) == hipSuccess && rb.pending() == 1);
    g_fail_copy_at = g_copy_calls;                            // the copy call itself fails
    CHECK(rb.add(db.data(), b.data(), 40, st) == hipErrorInvalidValue && rb.pending() == 0 && rb.offset() == 0);
    g_fail_copy_at = -1;
    CHECK(rb.finish(st) == hipSuccess && all_are(da, (char)0xEE) && all_are(db, (char)0xEE));   // the dropped batch reaches nobody
    CHECK(rb.add(db.data(), b.data(), 40, st) == hipSuccess && rb.pending() == 1 && rb.offset() == 48);
    CHECK(rb.finish(st) == hipSuccess && db == b && all_are(da, (char)0xEE));
    g_fail_copy_at = g_copy_calls;                            // ... of a 2-D piece
    CHECK(rb.add_2d(da.data(), a.data(), 12, 8, 4, st) == hipErrorInvalidValue && rb.pending() == 0 && rb.offset() == 0);
    g_fail_copy_at = -1;
    CHECK(rb.add(da.data(), a.data(), 48, st) == hipSuccess);
    g_fail_sync = true;                                       // the synchronisation fails: nothing is delivered, nothing is kept
    CHECK(rb.finish(st) == hipErrorUnknown && all_are(da, (char)0xEE) && rb.pending() == 0 && rb.offset() == 0);
    CHECK(hipStreamSynchronize(st) == hipSuccess);            // (the stand-in's own queue is drained before `a` goes)
    std::fill(da.begin(), da.end(), (char)0xEE);
    CHECK(rb.add(da.data(), a.data(), 48, st) == hipSuccess && rb.offset() == 48 && rb.finish(st) == hipSuccess && da == a);
    std::vector<char> far(70000, (char)0xEE);
    const std::vector<char> fsrc = pattern(70000, 8);
    g_fail_alloc = true;                                      // the growth fails: an error, an empty buffer, usable again
    CHECK(rb.add(far.data(), fsrc.data(), 70000, st) == hipErrorOutOfMemory && rb.capacity() == 0 && rb.pending() == 0);
    CHECK(rb.add(far.data(), fsrc.data(), 70000, st) == hipSuccess && rb.capacity() == 2 * (70000 + 64));
    CHECK(rb.finish(st) == hipSuccess && far == fsrc);
  }
  {
    ekf::ReadBack rb;                                         // 2-D: pitch 40 > 24 bytes per row, packed row-major at dst
    const std::vector<char> src = pattern(5 * 40, 9);
    std::vector<char> dst(5 * 24 + 8, (char)0xEE), one(7, (char)0xEE);
    CHECK(rb.add_2d(dst.data(), src.data(), 40, 24, 5, st) == hipSuccess && rb.offset() == 128);
    CHECK(rb.add(one.data(), src.data() + 3, 7, st) == hipSuccess && rb.offset() == 144 && rb.finish(st) == hipSuccess);
    bool rows = true;
    for (int r = 0; r < 5; ++r) rows = rows && memcmp(dst.data() + r * 24, src.data() + r * 40, 24) == 0;
    CHECK(rows && memcmp(one.data(), src.data() + 3, 7) == 0);
    for (int i = 0; i < 8; ++i) CHECK(dst[5 * 24 + i] == (char)0xEE);                            // nothing behind the block
  }
  CHECK(g_allocs_live == 0);
  printf("read-back: first use, edge, growth, failures, 2-D: %s\n", g_failed ? "DIFFERS" : "equal");
}

// ---- the input ring ---------------------------------------------------------------------------------------------------------
template <typename T>
static void check_input_ring() {
  const int cap = 10, calls = 6;
  hipStream_t st = nullptr;
  const int before = g_failed, made0 = g_events_made;
  {
    ekf::InputRing ring;
    ring.configure(sizeof(T), cap);
    // one "device" destination per call, so that every staged value can be looked at after the last synchronisation
    std::vector<std::vector<T>> dz(calls, std::vector<T>(2 * cap, T(-1))), dcam(calls, std::vector<T>(7, T(-1)));
    std::vector<std::vector<int>> didx(calls, std::vector<int>(cap, -1));
    const int waits0 = g_event_waits;
    for (int k = 0; k < calls; ++k) {
      const int M = (k % 2) ? cap : 3 + k;                   // a full list and short ones
      std::vector<T> z(2 * M), cam(7);
      std::vector<int> idx(M);
      for (int i = 0; i < 2 * M; ++i) z[i] = T(100 * k + i);
      for (int i = 0; i < M; ++i) idx[i] = 1000 * k + i;
      for (int i = 0; i < 7; ++i) cam[i] = T(10 * k + i) / T(4);
      const bool with_cam = k != 2;
      const int made = g_events_made;
      CHECK(ring.stage(st, M, dz[k].data(), z.data(), didx[k].data(), idx.data(), dcam[k].data(), with_cam ? cam.data() : nullptr) == hipSuccess);
      // the first kSlots calls wait for nothing and make one event each; the fifth waits for the first slot's event, the sixth for the second's
      CHECK(g_event_waits == waits0 + (k < ekf::InputRing::kSlots ? 0 : k - ekf::InputRing::kSlots + 1));
      CHECK(g_events_made == made + (k < ekf::InputRing::kSlots ? 1 : 0));
      if (k >= ekf::InputRing::kSlots) CHECK(g_last_waited == g_created[made0 + k - ekf::InputRing::kSlots]);
      // the copies of this call, in order: z, the index list, the camera pose
      const size_t base = g_queue.size() - (with_cam ? 3 : 2);
      CHECK(g_queue[base].dst == (char*)dz[k].data() && g_queue[base].width == 2 * M * sizeof(T));
      CHECK(g_queue[base + 1].dst == (char*)didx[k].data() && g_queue[base + 1].width == M * sizeof(int));
      CHECK(g_queue[base + 1].src == g_queue[base].src + 2 * cap * sizeof(T));
      if (with_cam) {
        CHECK(g_queue[base + 2].dst == (char*)dcam[k].data() && g_queue[base + 2].width == 7 * sizeof(T));
        CHECK(g_queue[base + 2].src == g_queue[base].src + cap * (2 * sizeof(T) + sizeof(int)));
      }
      // z, idx and cam of the caller go out of scope here: the ring has copied them into its slot
    }
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    for (int k = 0; k < calls; ++k) {                        // every call's values arrived, also those whose slot was used again
      const int M = (k % 2) ? cap : 3 + k;
      bool same = true;
      for (int i = 0; i < 2 * M; ++i) same = same && dz[k][i] == T(100 * k + i);
      for (int i = 0; i < M; ++i) same = same && didx[k][i] == 1000 * k + i;
      for (int i = 0; i < 7; ++i) same = same && dcam[k][i] == (k != 2 ? T(10 * k + i) / T(4) : T(-1));
      for (int i = 2 * M; i < 2 * cap; ++i) same = same && dz[k][i] == T(-1);
      CHECK(same);
    }
    CHECK(g_events_made == made0 + ekf::InputRing::kSlots && g_events_live == ekf::InputRing::kSlots);
    ring.release();                                          // the owner's tear-down: the events go once,
    CHECK(g_events_live == 0);
  }                                                          // ... the destructor finds none, the slots go with the ring
  CHECK(g_events_live == 0 && g_allocs_live == 0);
  printf("input ring (%d-byte scalars): %d calls on %d slots: %s\n", (int)sizeof(T), calls, ekf::InputRing::kSlots,
         g_failed == before ? "equal" : "DIFFERS");
}

// ---- the launch profiler ----------------------------------------------------------------------------------------------------
static void check_profiler() {
  const int before = g_failed, made0 = g_events_made;
  enum { K_A, K_DOM, K_B, K_DOM2, K_COUNT };
  using Prof = ekf::LaunchProfiler<K_COUNT>;
  {
    Prof p(K_DOM, K_DOM2);
    for (int kid = 0; kid < K_COUNT; ++kid) {
      const bool dom = kid == K_DOM || kid == K_DOM2;
      p.mode = 0; CHECK(!p.on(kid));
      p.mode = 1; CHECK(p.on(kid) == dom);
      p.mode = 2; CHECK(p.on(kid));
      p.mode = 3;
      for (p.frame_seq = 0; p.frame_seq < 17; ++p.frame_seq) CHECK(p.on(kid) == (dom && p.frame_seq % Prof::kSamplePeriod == 0));
    }
    p.frame_seq = 0;
    p.mode = 0;
    { Prof::Scope sc(p, K_DOM, nullptr); CHECK(!sc.on); }
    CHECK(g_events_made == made0);                            // off: no event call at all
    p.mode = 1;
    { Prof::Scope sc(p, K_DOM, nullptr); CHECK(sc.on); if (sc.on) p.work[K_DOM] += 8.0; }
    { Prof::Scope sc(p, K_A, nullptr); CHECK(!sc.on); }
    CHECK(g_events_made == made0 + 2);
    double ms = -1.0; long long cnt = -1;
    p.read(K_DOM, &ms, &cnt);
    CHECK(ms == 0.0 && cnt == 0);                             // pending until resolved
    const int syncs = g_stream_syncs;
    p.resolve(nullptr, nullptr, nullptr);
    CHECK(g_stream_syncs == syncs + 2);                       // the main and the side stream; no gather stream
    p.read(K_DOM, &ms, &cnt);
    CHECK(ms == 1.5 && cnt == 1 && p.work[K_DOM] == 8.0);
    p.resolve(nullptr, nullptr, nullptr);
    CHECK(g_stream_syncs == syncs + 2);                       // nothing pending: nothing drained
    p.mode = 2;
    { Prof::Scope sc(p, K_B, nullptr); }
    CHECK(g_events_made == made0 + 2);                        // the pair came out of the pool
    { Prof::Scope sc(p, K_A, nullptr); }
    CHECK(g_events_made == made0 + 4);
    p.frame_seq = 5;
    p.resolve(nullptr, nullptr, nullptr);
    p.reset();
    p.read(K_B, &ms, &cnt);
    CHECK(ms == 0.0 && cnt == 0 && p.work[K_DOM] == 0.0 && p.frame_seq == 0 && p.mode == 2);
    { Prof::Scope sc(p, K_B, nullptr); }                      // one pair pending, one in the pool
    CHECK(g_events_live == 4);
    p.release();
    CHECK(g_events_live == 0);
  }
  CHECK(g_events_live == 0);
  printf("launch profiler: modes 0..3, pool, resolve, reset, release: %s\n", g_failed == before ? "equal" : "DIFFERS");
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) replay(argv[i]);
  check_readback();
  check_input_ring<float>();
  check_input_ring<double>();
  check_profiler();
  if (g_failed) { printf("%d checks DIFFER\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
