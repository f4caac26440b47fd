// The filter's per-feature host records (plain C++17, no HIP): one column per field of a Patch, all of one length.
// Only the operations below change a column, and each of them changes all columns together, so the lengths cannot drift
// apart; readers go through size() and the per-feature getters.  Offsets, codings and real indices are kept as whole int
// columns because the filter uploads them as they are (sync_layout, export_points_table).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace ekf {

class FeatureTable {
 public:
  struct Columns {
    std::vector<int> pos, coding;                   // first state row; 0: inverse depth (6 states), 1: XYZ (3 states)
    std::vector<int> real_index, n_find, n_tot;     // Patch::real_index (vR.cpp:148, 318-319), n_find, n_tot (Patch.cpp:85-93, 145, 218)
    std::vector<float> center;                      // u, v per feature (Patch.cpp:253, 279)
    std::vector<unsigned char> in_innovation, remove_flag;   // isInInnovation; the sticky removeFlag
  };
  // What a set of removals and conversions makes of the table: the new columns, and per new state row the old row it is
  // taken from (`msrc`) and, for the three rows of a feature that is converted, 3 * old feature + e (`mconv`; else -1).
  struct Compaction {
    Columns cols;
    std::vector<int> msrc, mconv;
  };

  int size() const { return (int)c_.pos.size(); }
  int next_real_index() const { return patchnumbre_; }

  // A new inverse-depth feature at state row `row`, seen at (u, v): found once in one frame (Patch.cpp:85-93)
  void add(int row, float u, float v) {
    c_.pos.push_back(row);
    c_.coding.push_back(0);
    c_.real_index.push_back(patchnumbre_++);
    c_.n_find.push_back(1);
    c_.n_tot.push_back(1);
    c_.center.push_back(u);
    c_.center.push_back(v);
    c_.in_innovation.push_back(0);
    c_.remove_flag.push_back(0);
  }

  // The table without the features of `rm` and with those of `cv` as XYZ features, behind `camera_dim` camera rows.  The
  // table itself is left alone: the filter adopts the result once the device has followed.
  template <typename Mask>
  Compaction compacted(const Mask& rm, const Mask& cv, int camera_dim) const {
    Compaction r;
    r.msrc.reserve(camera_dim + 6 * (size_t)size());
    r.mconv.reserve(camera_dim + 6 * (size_t)size());
    for (int i = 0; i < camera_dim; ++i) { r.msrc.push_back(i); r.mconv.push_back(-1); }
    for (int i = 0; i < size(); ++i) {
      if (rm[i]) continue;
      const int fs = c_.coding[i] ? 3 : 6;
      r.cols.pos.push_back((int)r.msrc.size());
      r.cols.real_index.push_back(c_.real_index[i]);
      r.cols.n_find.push_back(c_.n_find[i]);
      r.cols.n_tot.push_back(c_.n_tot[i]);
      r.cols.center.push_back(c_.center[2 * i]);
      r.cols.center.push_back(c_.center[2 * i + 1]);
      r.cols.in_innovation.push_back(c_.in_innovation[i]);
      r.cols.remove_flag.push_back(c_.remove_flag[i]);
      if (cv[i]) {
        for (int e = 0; e < 3; ++e) { r.msrc.push_back(c_.pos[i]); r.mconv.push_back(i * 3 + e); }
        r.cols.coding.push_back(1);
      } else {
        for (int e = 0; e < fs; ++e) { r.msrc.push_back(c_.pos[i] + e); r.mconv.push_back(-1); }
        r.cols.coding.push_back(c_.coding[i]);
      }
    }
    return r;
  }
  void adopt(Columns&& cols) { c_ = std::move(cols); }

  // The device's track bits of one predict / measure, one byte per feature: bit 0 is the visibility at the last one, bit 1
  // says that rho <= 0 was seen since the last fold -- which sets the removal flag and never clears it.
  template <typename Bits>
  void fold_track(const Bits& b) {
    for (int i = 0; i < size(); ++i) {
      c_.in_innovation[i] = b[i] & 1;
      c_.remove_flag[i] |= (b[i] >> 1) & 1;
    }
  }
  // Patch::findMatch of a searched feature: n_tot + 1 (Patch.cpp:218), the centre becomes the matched pixel or (-1, -1)
  // (:253, 279), a failed search clears isInInnovation (:281)
  void searched(int i, bool found, float u, float v) {
    c_.n_tot[i] += 1;
    c_.center[2 * i] = found ? u : -1.f;
    c_.center[2 * i + 1] = found ? v : -1.f;
    if (!found) c_.in_innovation[i] = 0;
  }
  void count_found(int i) { c_.n_find[i] += 1; }          // update_quality_index (Patch.cpp:145)
  void flag_removal(int i) { c_.remove_flag[i] = 1; }

  // setters of the C ABI: a negative int (a null centre) leaves the field as it is
  void set_meta(int i, int real_index, int n_find) {
    if (real_index >= 0) c_.real_index[i] = real_index;
    if (n_find >= 0) c_.n_find[i] = n_find;
  }
  void set_track(int i, int n_tot, int in_innovation, const float* center, int remove_flag) {
    if (n_tot >= 0) c_.n_tot[i] = n_tot;
    if (in_innovation >= 0) c_.in_innovation[i] = in_innovation ? 1 : 0;
    if (center) { c_.center[2 * i] = center[0]; c_.center[2 * i + 1] = center[1]; }
    if (remove_flag >= 0) c_.remove_flag[i] = remove_flag ? 1 : 0;
  }

  int pos(int i) const { return c_.pos[i]; }
  int coding(int i) const { return c_.coding[i]; }
  int real_index(int i) const { return c_.real_index[i]; }
  int n_find(int i) const { return c_.n_find[i]; }
  int n_tot(int i) const { return c_.n_tot[i]; }
  const float* center(int i) const { return &c_.center[2 * (size_t)i]; }
  bool in_innovation(int i) const { return c_.in_innovation[i] != 0; }
  bool remove_flag(int i) const { return c_.remove_flag[i] != 0; }
  const Columns& columns() const { return c_; }          // whole columns, for uploads and the getters that copy them out

 private:
  Columns c_;
  int patchnumbre_ = 1;                                  // the next real_index (vR.cpp:148)
};

}  // namespace ekf
