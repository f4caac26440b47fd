// The stamp rule of csrc/ekf_mesh_stamp.hpp beside the rules it replaced, on the host: every sequence of up to
// LENGTH operations on a fusion handle's mesh chain is run through both, and after every step both must agree on which of
// sources 0..3 resolve, on the class of message each failure gets, and on whether the components, the smooth adjacency, the
// smooth result, the simplify result and the texture are current.  No HIP, no device: the operations are what the stage structs
// do to their bookkeeping, and nothing else.
//
// `Old` restates the bookkeeping before the stamps literally: a view is (source, serial, prune); TsdfSmooth::runs and
// TsdfSimplify::runs are carried beside it; TsdfSimplify keeps smooth_run, TsdfTexture run_id and from; TsdfComponents keeps
// comp_serial and prune_serial, components() clears prune_valid, and a prune finds the components first when it lacks them.  The
// resolution is the chain smooth_source -> simplify_source -> texture_source with smooth_result, simplify_result and
// texture_current threaded through it, as ekf_capi.hip had it.
//
// Usage: mesh_stamp_check [LENGTH]     (default 6; prints the number of steps checked and "ok")
#include <cstdio>
#include <cstdlib>

#include "../ekf-monoslam_for_3d-reconstruction_amd/csrc/ekf_mesh_stamp.hpp"

typedef unsigned long long ull;

// the class of a resolution's message: the text after "who: "
enum Msg { kOk, kNoWeld, kNeedsPrune, kNeedsSmooth, kNeedsSimplify };

// ---- the rules before the stamps ---------------------------------------------------------------------------------------------
struct OldView {
  int source = 0;
  ull serial = 0, prune = 0;
};

struct Old {
  ull changes = 0;                                                     // TsdfFusion
  bool w_valid = false;                                                // TsdfMesh
  ull weld_changes = 0, serial = 0;
  bool comp_valid = false, prune_valid = false;                        // TsdfComponents
  ull comp_serial = 0, prune_serial = 0, prunes = 0;
  OldView adj, res;                                                    // TsdfSmooth
  bool adj_valid = false, res_valid = false;
  ull runs = 0;
  OldView src;                                                         // TsdfSimplify
  int from = 0;
  ull smooth_run = 0, simp_runs = 0;
  bool simp_valid = false;
  OldView t_src;                                                       // TsdfTexture
  int t_from = 0;
  ull run_id = 0;
  bool begun = false;

  static bool same(const OldView& a, const OldView& b) { return a.source == b.source && a.serial == b.serial && a.prune == b.prune; }
  bool mesh_current() const { return w_valid && weld_changes == changes; }
  bool have_components() const { return comp_valid && comp_serial == serial; }
  bool have_pruned() const { return prune_valid && prune_serial == serial; }
  OldView view() const { return OldView{0, serial, 0}; }
  OldView pruned_view() const { return OldView{1, serial, prunes}; }
  bool have_adjacency(const OldView& s) const { return adj_valid && same(adj, s); }
  bool have_result(const OldView& s) const { return res_valid && same(res, s); }
  bool simp_have_result(int f, const OldView& s, ull run) const {
    return simp_valid && from == f && same(src, s) && (f != 2 || smooth_run == run);
  }

  Msg smooth_source(int source, OldView* s) const {
    if (!mesh_current()) return kNoWeld;
    if (source == 1 && !have_pruned()) return kNeedsPrune;
    *s = source == 0 ? view() : pruned_view();
    return kOk;
  }
  bool smooth_result(OldView* r) const {
    OldView s;
    if (!res_valid || smooth_source(res.source, &s) != kOk || !have_result(s)) return false;
    *r = s;                                                            // the result's view is its source's, with other rows
    return true;
  }
  Msg simplify_source(int source, OldView* s, ull* run) const {
    *run = 0;
    if (source != 2) return smooth_source(source, s);
    if (!mesh_current()) return kNoWeld;
    if (!smooth_result(s)) return kNeedsSmooth;
    *run = runs;
    return kOk;
  }
  bool simplify_result() const {
    OldView s;
    ull run = 0;
    return simp_valid && simplify_source(from, &s, &run) == kOk && simp_have_result(from, s, run);
  }
  Msg texture_source(int source, OldView* s, ull* run) const {
    if (source != 3) return simplify_source(source, s, run);
    if (!simplify_result()) return kNeedsSimplify;
    *s = OldView{3, src.serial, src.prune};
    *run = simp_runs;
    return kOk;
  }
  bool texture_current() const {
    OldView s;
    ull run = 0;
    return begun && texture_source(t_from, &s, &run) == kOk && same(t_src, s) && !(t_from >= 2 && run_id != run);
  }

  void weld(bool fail) {
    w_valid = false;
    ++serial;
    if (fail) return;
    weld_changes = changes;
    w_valid = true;
  }
  void components(bool fail) {
    comp_valid = prune_valid = false;
    if (fail) return;
    comp_serial = serial;
    comp_valid = true;
  }
  void prune(int fail) {                                               // 1: an allocation fails; 2: the flags launch fails
    if (!have_components()) components(false);
    prune_valid = false;
    ++prunes;
    if (fail == 2) comp_valid = false;
    if (fail) return;
    prune_serial = serial;
    prune_valid = true;
  }
  void smooth(const OldView& s, bool fail) {
    res_valid = false;
    ++runs;
    if (fail) return;
    if (!have_adjacency(s)) {
      adj = s;
      adj_valid = true;
    }
    res = s;
    res_valid = true;
  }
  void simplify(const OldView& s, int f, ull run, bool fail) {
    simp_valid = false;
    ++simp_runs;
    if (fail) return;
    src = s;
    from = f;
    smooth_run = run;
    simp_valid = true;
  }
  void texture(const OldView& s, int f, ull run) {
    begun = false;
    t_src = s;
    t_from = f;
    run_id = run;
    begun = true;
  }
};

// ---- the stamps: what the stage structs do to ekf::MeshStamps, and ekf_capi.hip's table of messages ------------------------------
struct New {
  ull changes = 0;
  ekf::MeshStamps st;

  Msg source(int s, ull* id) const {
    *id = st.current(s, changes);
    if (*id != 0) return kOk;
    if (s != 3 && st.current(0, changes) == 0) return kNoWeld;
    return s == 1 ? kNeedsPrune : (s == 2 ? kNeedsSmooth : kNeedsSimplify);
  }
  void weld(bool fail) {
    st.begin(st.weld);
    if (fail) return;
    st.weld_changes = changes;
    st.weld.valid = true;
  }
  void components(ull weld_id, bool fail) {
    st.comp.valid = st.pruned.valid = false;
    if (!fail) st.made(st.comp, weld_id, 0);
  }
  void prune(ull weld_id, int fail) {
    if (!st.comp.made_from(weld_id)) components(weld_id, false);
    st.begin(st.pruned);
    if (fail == 2) st.comp.valid = false;
    if (!fail) st.made(st.pruned, weld_id, 0);
  }
  void smooth(ull id, int s, bool fail) {
    st.begin(st.smooth);
    if (fail) return;
    if (!st.adj.made_from(id)) st.made(st.adj, id, s);
    st.made(st.smooth, id, s);
  }
  void simplify(ull id, int s, bool fail) {
    st.begin(st.simp);
    if (!fail) st.made(st.simp, id, s);
  }
  void texture(ull id, int s) {
    st.tex.valid = false;
    st.made(st.tex, id, s);
  }
};

// ---- the operations --------------------------------------------------------------------------------------------------------------
// 0 a volume change; 1, 2 weld and a failing one; 3, 4 components; 5, 6, 7 prune, failing at an allocation, failing at the flags;
// 8..11 smooth from 0 and 1, then failing; 12..17 simplify from 0, 1, 2, then failing; 18..21 texture begin from 0..3.  (A failing
// ekf_texture_begin fails before it touches the texture begun before: no operation.)
constexpr int kOps = 22;
static const char* const kNames[kOps] = {"change", "weld", "weld!", "components", "components!", "prune", "prune!", "prune!!",
                                         "smooth0", "smooth1", "smooth0!", "smooth1!", "simplify0", "simplify1", "simplify2",
                                         "simplify0!", "simplify1!", "simplify2!", "texture0", "texture1", "texture2", "texture3"};

static ull g_steps = 0, g_resolved[4] = {0, 0, 0, 0}, g_msg[5] = {0, 0, 0, 0, 0}, g_textured[4] = {0, 0, 0, 0}, g_noop = 0;
static int g_path[16];

static void fail(int depth, const char* what, int source) {
  std::printf("DIFFERS: %s (source %d) after", what, source);
  for (int i = 0; i <= depth; ++i) std::printf(" %s", kNames[g_path[i]]);
  std::printf("\n");
  std::exit(1);
}

// false: the operation's source does not resolve, so it is refused and both sides stay as they were
static bool apply(Old& o, New& n, int op, int depth) {
  OldView s;
  ull run = 0, id = 0;
  if (op == 0) {
    ++o.changes;
    ++n.changes;
  } else if (op <= 2) {
    o.weld(op == 2);
    n.weld(op == 2);
  } else if (op <= 7) {                                                // the entry points ask for a current weld first
    const bool ok = o.mesh_current();
    if (ok != (n.source(0, &id) == kOk)) fail(depth, "the weld", 0);
    if (!ok) { ++g_noop; return false; }
    if (op <= 4) { o.components(op == 4); n.components(id, op == 4); }
    else { o.prune(op - 5); n.prune(id, op - 5); }
  } else {
    const int source = op <= 11 ? (op - 8) & 1 : (op <= 17 ? (op - 12) % 3 : op - 18);
    const bool failing = op <= 11 ? op >= 10 : op >= 15;
    const Msg mo = op <= 11 ? o.smooth_source(source, &s) : (op <= 17 ? o.simplify_source(source, &s, &run) : o.texture_source(source, &s, &run));
    if (mo != n.source(source, &id)) fail(depth, "the source of a run", source);
    if (mo != kOk) { ++g_noop; return false; }
    if (op <= 11) { o.smooth(s, failing); n.smooth(id, source, failing); }
    else if (op <= 17) { o.simplify(s, source, run, failing); n.simplify(id, source, failing); }
    else { o.texture(s, source, run); n.texture(id, source); }
  }
  return true;
}

static void compare(const Old& o, const New& n, int depth) {
  ++g_steps;
  for (int source = 0; source < 4; ++source) {
    OldView s;
    ull run = 0, id = 0;
    const Msg mo = o.texture_source(source, &s, &run), mn = n.source(source, &id);
    if (mo != mn) fail(depth, "whether a source resolves, or its message", source);
    ++g_msg[mo];
    if (mo == kOk) ++g_resolved[source];
    if (source < 2) {                                                  // the adjacency, as a smooth run of this source would ask for it
      const bool ao = mo == kOk && o.have_adjacency(s), an = n.st.adj.made_from(id);
      if (ao != an) fail(depth, "the smooth adjacency", source);
    }
  }
  const ekf::MeshStamps& st = n.st;
  OldView r;
  if ((o.mesh_current() && o.have_components()) != st.has(st.comp, n.changes)) fail(depth, "the components", 0);
  const bool smoothed = o.smooth_result(&r);
  if (smoothed != (st.current(2, n.changes) != 0)) fail(depth, "the smooth result", 2);
  if (smoothed && o.res.source != st.smooth.from) fail(depth, "the source of the smooth result", 2);
  const bool simplified = o.simplify_result();
  if (simplified != (st.current(3, n.changes) != 0)) fail(depth, "the simplify result", 3);
  if (simplified && o.from != st.simp.from) fail(depth, "the source of the simplify result", 3);
  const bool textured = o.texture_current();
  if (textured != st.has(st.tex, n.changes)) fail(depth, "the texture", o.t_from);
  if (textured && o.t_from != st.tex.from) fail(depth, "the source of the texture", o.t_from);
  if (textured) ++g_textured[o.t_from];
}

static void walk(const Old& o, const New& n, int depth, int length) {
  for (int op = 0; op < kOps; ++op) {
    Old o2 = o;
    New n2 = n;
    g_path[depth] = op;
    const bool done = apply(o2, n2, op, depth);
    compare(o2, n2, depth);
    // what follows a refused operation follows the sequence without it, which is one of the shorter sequences: not walked again
    if (done && depth + 1 < length) walk(o2, n2, depth + 1, length);
  }
}

int main(int argc, char** argv) {
  const int length = argc > 1 ? std::atoi(argv[1]) : 6;
  if (length < 1 || length > 16) {
    std::printf("LENGTH in 1..16\n");
    return 2;
  }
  walk(Old(), New(), 0, length);
  std::printf("%d operations, sequences of up to %d: %llu steps checked, %llu of them refused\n", kOps, length, g_steps, g_noop);
  std::printf("resolved: source 0 %llu, 1 %llu, 2 %llu, 3 %llu\n", g_resolved[0], g_resolved[1], g_resolved[2], g_resolved[3]);
  std::printf("messages: ok %llu, no weld %llu, needs prune %llu, needs smooth %llu, needs simplify %llu\n", g_msg[0], g_msg[1], g_msg[2],
              g_msg[3], g_msg[4]);
  std::printf("a current texture of source 0 %llu, 1 %llu, 2 %llu, 3 %llu\n", g_textured[0], g_textured[1], g_textured[2], g_textured[3]);
  std::printf("ok\n");
  return 0;
}
