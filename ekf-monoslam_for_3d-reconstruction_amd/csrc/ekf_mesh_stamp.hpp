// Which mesh a source number means, and whether a result made earlier is still the result of that mesh.
// Plain C++, no HIP: tools/mesh_stamp_check.cpp runs it on the host beside the rules it replaced.
//
// The fusion handle issues stamps from one counter; 0 is "none".  Every attempt to make a mesh (a weld, a prune, a smooth run,
// a simplify run) takes a fresh stamp before its first allocation, so a failed attempt retires the old mesh too.  A view
// carries the stamp of its mesh as `id`; whatever is made from a view remembers that stamp as `src_id`.  A result is current
// iff it is valid and its src_id is the id of the current view of its source.  The weld alone has no source: it is current
// iff it is valid and the volume has not changed since (TsdfFusion::changes).
#pragma once

namespace ekf {

// What a stage keeps of its last attempt.
struct MeshStage {
  unsigned long long id = 0;          // the stamp of the attempt: the name of the mesh it made, if it made one
  unsigned long long src_id = 0;      // the stamp of the view the result was made from
  int from = 0;                       // the source number that view was asked by: 0 the weld, 1 the pruned, 2 the smoothed,
                                      // 3 the simplified mesh; always below the stage's own number, so `current` ends
  bool valid = false;

  bool made_from(unsigned long long view_id) const { return valid && view_id != 0 && src_id == view_id; }
};

struct MeshStamps {
  unsigned long long issued = 0;      // the last stamp
  unsigned long long weld_changes = 0;           // TsdfFusion::changes when the weld was made
  MeshStage weld, comp, pruned, adj, smooth, simp, tex;        // comp, adj and tex make no mesh: their id stays 0

  // An attempt to make a mesh begins: its old result is retired, and what was made from it is current no longer.
  void begin(MeshStage& s) {
    s.valid = false;
    s.id = ++issued;
  }
  void made(MeshStage& s, unsigned long long src_id, int from) {
    s.src_id = src_id;
    s.from = from;
    s.valid = true;
  }

  // The stamp of the mesh that `source` (0..3) means now, or 0 when the handle holds none.
  unsigned long long current(int source, unsigned long long changes) const {
    if (!weld.valid || weld_changes != changes) return 0;
    if (source == 0) return weld.id;
    const MeshStage& s = source == 1 ? pruned : (source == 2 ? smooth : simp);
    return has(s, changes) ? s.id : 0;
  }
  // Whether a result is that of the current view of its source.
  bool has(const MeshStage& s, unsigned long long changes) const { return s.valid && s.made_from(current(s.from, changes)); }
};

}  // namespace ekf
