// Host check of csrc/ekf_buffers.hpp: Buf and IndexedMeshBufs with a counting malloc / free allocator, no device.  Built with
// -fsanitize=address,undefined by tests/test_buffers_host.py; a leak, a double free or a use after free ends the run.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_buffers.hpp"

static int g_allocs = 0, g_frees = 0;
static bool g_fail_next = false;
static int g_fail_in = 0;                        // n > 0: the n-th allocation from here fails
static size_t g_last_bytes = 0;

struct CountingAlloc {
  static hipError_t alloc(void** p, size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) g_fail_next = true;
    if (g_fail_next) { g_fail_next = false; *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes);
    if (!*p) return hipErrorOutOfMemory;
    ++g_allocs;
    g_last_bytes = bytes;
    return hipSuccess;
  }
  static void release(void* p) { free(p); ++g_frees; }
};
using HostBuf = ekf::Buf<double, CountingAlloc>;

static int g_failed = 0;
#define CHECK(cond) \
  do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static_assert(!std::is_copy_constructible<HostBuf>::value && !std::is_copy_assignable<HostBuf>::value, "move-only");

// IndexedMeshBufs::grow: all six buffers or none.
using HostMesh = ekf::IndexedMeshBufs<CountingAlloc>;
static_assert(!std::is_copy_constructible<HostMesh>::value && !std::is_copy_assignable<HostMesh>::value, "move-only");

struct MeshState {                               // the six pointers and capacities
  const void* p[6];
  size_t cap[6];
  explicit MeshState(const HostMesh& m)
      : p{m.xyz, m.key, m.grey, m.bgr, m.normal, m.faces},
        cap{m.xyz.capacity(), m.key.capacity(), m.grey.capacity(), m.bgr.capacity(), m.normal.capacity(), m.faces.capacity()} {}
  bool operator==(const MeshState& o) const {
    for (int i = 0; i < 6; ++i)
      if (p[i] != o.p[i] || cap[i] != o.cap[i]) return false;
    return true;
  }
  // room for nv vertices and ncorner face indices; bgr and normal exactly `colour` and `normals` say, empty otherwise
  bool holds(size_t nv, size_t ncorner, bool colour, bool normals) const {
    return cap[0] >= nv * 3 && cap[1] >= nv && cap[2] >= nv && cap[5] >= ncorner && (colour ? cap[3] >= nv * 3 : !p[3] && cap[3] == 0) &&
           (normals ? cap[4] >= nv * 3 : !p[4] && cap[4] == 0);
  }
};

static void mesh_bufs() {
  const int a0 = g_allocs, f0 = g_frees;
  {
    HostMesh z;
    CHECK(z.grow(0, 0, true, true) == hipSuccess && g_allocs == a0);           // nothing asked, nothing done
    CHECK(MeshState(z).holds(0, 0, false, false) && !z.xyz && !z.faces);

    HostMesh m;
    CHECK(m.grow(10, 12, true, true) == hipSuccess);                           // 1. a small mesh with colour and normals
    CHECK(g_allocs == a0 + 6 && g_frees == f0 && MeshState(m).holds(10, 12, true, true));
    CHECK(m.n_vert == 0 && m.n_tri == 0 && !m.has_normals);                    // the counts are the holder's to set
    m.xyz[29] = 1.0; m.key[9] = 1; m.grey[9] = 1; m.bgr[29] = 1; m.normal[29] = 1.f; m.faces[11] = 1;

    const MeshState s1(m);
    CHECK(m.grow(4, 6, true, true) == hipSuccess);                             // 2. a smaller one: nothing allocated, nothing moved
    CHECK(g_allocs == a0 + 6 && g_frees == f0 && MeshState(m) == s1);

    g_fail_next = true;                                                        // 3. a larger one, the first allocation failing ...
    CHECK(m.grow(20, 30, true, true) == hipErrorOutOfMemory);
    CHECK(MeshState(m) == s1 && g_allocs == a0 + 6 && g_frees == f0);
    int made = 0;
    for (int k = 1; k <= 6; ++k) {                                             // ... then each of the six in turn, the last included
      g_fail_in = k;
      CHECK(m.grow(20, 30, true, true) == hipErrorOutOfMemory);
      made += k - 1;                                                           // the k - 1 new buffers before it are freed again
      CHECK(MeshState(m) == s1 && g_fail_in == 0 && !g_fail_next);
      CHECK(g_allocs == a0 + 6 + made && g_frees == f0 + made);
    }
    CHECK(m.xyz[29] == 1.0 && m.faces[11] == 1);                               // the previous mesh is intact

    CHECK(m.grow(20, 30, true, true) == hipSuccess);                           // 4. again, without the failure
    CHECK(MeshState(m).holds(20, 30, true, true) && g_allocs == a0 + 12 + made && g_frees == f0 + 6 + made);
    m.xyz[59] = 2.0; m.faces[29] = 2;

    CHECK(m.grow(3, 40, true, true) == hipSuccess);                            // one buffer too small: all six are replaced together
    CHECK(MeshState(m).holds(3, 40, true, true) && m.xyz.capacity() == 9 && g_allocs == a0 + 18 + made && g_frees == f0 + 12 + made);
    CHECK(m.grow(50, 60, true, false) == hipSuccess);                          // grown without normals: none are kept
    CHECK(MeshState(m).holds(50, 60, true, false) && g_allocs == a0 + 23 + made && g_frees == f0 + 18 + made);

    HostMesh n;                                                                // 5. a second one without colour and normals
    CHECK(n.grow(5, 9, false, false) == hipSuccess);
    CHECK(MeshState(n).holds(5, 9, false, false) && g_allocs == a0 + 27 + made);

    HostMesh o(std::move(n));                                                  // moves as a whole
    CHECK(MeshState(o).holds(5, 9, false, false) && MeshState(n).holds(0, 0, false, false) && !n.xyz);
  }
  CHECK(g_allocs == a0 + 42 && g_frees == f0 + 42);
}

int main() {
  {
    HostBuf b;
    CHECK(!b && b.capacity() == 0);                                  // default: empty
    CHECK(b.reserve(0) == hipSuccess && !b && g_allocs == 0);        // nothing asked, nothing done

    CHECK(b.reserve(10) == hipSuccess);
    CHECK(b && b.capacity() == 10 && g_allocs == 1 && g_frees == 0 && g_last_bytes == 10 * sizeof(double));
    double* p0 = b;
    for (int i = 0; i < 10; ++i) b[i] = i;                            // (the sanitizer watches the block)
    CHECK(*(b + 9) == 9.0);

    CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && b.reserve(7, 1000) == hipSuccess);
    CHECK(static_cast<double*>(b) == p0 && b.capacity() == 10 && g_allocs == 1 && g_frees == 0);   // fits: pointer kept, grow_to ignored

    CHECK(b.reserve(11, 64) == hipSuccess);                           // beyond: one free, one allocation of max(need, grow_to)
    CHECK(b.capacity() == 64 && g_allocs == 2 && g_frees == 1 && g_last_bytes == 64 * sizeof(double));
    CHECK(b.reserve(100, 80) == hipSuccess);
    CHECK(b.capacity() == 100 && g_allocs == 3 && g_frees == 2);
    b[99] = 1.0;

    g_fail_next = true;                                               // a failed allocation: the error comes back, the buffer is empty
    CHECK(b.reserve(200) == hipErrorOutOfMemory);
    CHECK(!b && b.capacity() == 0 && g_allocs == 3 && g_frees == 3);
    CHECK(b.reserve(5) == hipSuccess && b.capacity() == 5 && g_allocs == 4);   // ... and usable again

    double* p1 = b;
    HostBuf c(std::move(b));                                          // move construction: ownership moves, nothing is freed
    CHECK(static_cast<double*>(c) == p1 && c.capacity() == 5 && !b && b.capacity() == 0 && g_frees == 3);

    HostBuf d;
    CHECK(d.reserve(8) == hipSuccess && g_allocs == 5);
    double* p2 = d;
    c = std::move(d);                                                 // move assignment: the target's old block is freed, once
    CHECK(static_cast<double*>(c) == p2 && c.capacity() == 8 && !d && d.capacity() == 0 && g_frees == 4);
    HostBuf& cref = c;
    c = std::move(cref);                                              // onto itself: nothing happens
    CHECK(static_cast<double*>(c) == p2 && c.capacity() == 8 && g_frees == 4);
    c[7] = 2.0;

    HostBuf e;
    CHECK(e.reserve(2) == hipSuccess && g_allocs == 6);
    e.reset();
    CHECK(!e && e.capacity() == 0 && g_frees == 5);
    e.reset();                                                        // (twice is once)
    CHECK(g_frees == 5);
  }                                                                   // b, d, e empty; c holds a block
  CHECK(g_allocs == 6 && g_frees == 6);
  mesh_bufs();
  CHECK(g_allocs == 48 && g_frees == 48);       // 6 above, 42 in mesh_bufs; nothing leaked
  if (g_failed) return 1;
  printf("allocs=%d frees=%d ok\n", g_allocs, g_frees);
  return 0;
}
