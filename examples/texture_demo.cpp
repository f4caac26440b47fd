// A texture atlas of a simplified mesh through include/vslam_filter_hip.hpp's TsdfVolumeHip::textureBegin / textureAddViewHost /
// textureFinish.  The volume is written directly: the analytic sphere of radius 1.25 round the world
// origin on a 17 x 15 x 13 grid.  The demo welds, simplifies at cells of 2 voxels, textures the result at a patch of 8 texels
// from two views of constant grey (one on the -z axis, one on the +z axis, each behind its own ray cast of the volume), and
// holds a few invariants: the atlas has the side the contract gives, every textured triangle's texels carry exactly its view's
// constant, every other triangle's the blend of its vertices' grey (128 everywhere), padding is 0, the UV corners are centres of
// texels, and the simplified mesh is what it was.  It writes the 3-channel atlas as atlas.ppm (or the path given).  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

typedef TsdfVolumeHip::IndexedMesh Mesh;

int main(int argc, char** argv) {
  const int nx = 17, ny = 15, nz = 13;
  const double origin[3] = {-2.0, -1.75, -1.5}, voxel = 0.25, trunc = 0.5, radius = 1.25;
  TsdfVolumeHip vol(nx, ny, nz, origin, voxel, trunc);
  const size_t n = (size_t)nx * ny * nz;
  std::vector<float> sum(n);
  std::vector<unsigned short> cnt(n, 1);
  std::vector<unsigned int> gsum(n, 128);
  for (int k = 0; k < nz; ++k)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const double x = origin[0] + i * voxel, y = origin[1] + j * voxel, z = origin[2] + k * voxel;
        const double d = (std::sqrt(x * x + y * y + z * z) - radius) / trunc;
        sum[(size_t)i + (size_t)nx * ((size_t)j + (size_t)ny * (size_t)k)] = (float)std::max(-1.0, std::min(1.0, d));
      }
  if (ekf_fusion_set_volume(vol.handle(), sum.data(), cnt.data(), gsum.data(), 1) != EKF_OK) return 2;

  vol.profile(true);
  vol.weld(1);
  const Mesh coarse = vol.simplify(2.0 * voxel);
  const int P = 8, B = P + 2, W = 64, H = 48;
  const int side = vol.textureBegin(3, P, 3);               // 3 channels over a plain volume: grey, replicated
  int Q = 0;
  while ((size_t)Q * Q < (coarse.triangles() + 1) / 2) ++Q;
  bool ok = side == Q * B && coarse.triangles() > 0;

  const double K[4] = {60.0, 60.0, 31.5, 23.5};
  const double front[7] = {0.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0}, back[7] = {0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 0.0};   // half a turn about y
  const unsigned char shade[2] = {80, 200};
  unsigned long long won[2];
  for (int v = 0; v < 2; ++v) {
    const std::vector<unsigned char> img((size_t)W * H, shade[v]);
    const TsdfVolumeHip::Occlusion behind(2.0, 6.5);           // the wrapper renders the view itself; tol: the cell
    won[v] = vol.textureAddViewHost(img.data(), 1, W, H, K, v ? back : front, &behind);
  }
  const TsdfVolumeHip::TextureAtlas peek = vol.texture();
  const TsdfVolumeHip::TextureAtlas t = vol.textureFinish();
  std::printf("%zu triangles, atlas %d x %d x %d, the views won %llu and %llu, %llu textured\n", coarse.triangles(), t.side, t.side,
              t.channels, won[0], won[1], t.n_textured);
  ok = ok && t.channels == 3 && t.triangles() == coarse.triangles() && won[0] > 0 && won[1] > 0 && t.n_textured == won[0] + won[1];
  ok = ok && peek.n_textured == t.n_textured && peek.view == t.view && peek.score == t.score && peek.uv == t.uv;

  // every texel against its owner
  size_t wrong = 0, padding = 0;
  for (int y = 0; y < side; ++y)
    for (int x = 0; x < side; ++x) {
      const int a = x % B, b = y % B;
      const size_t tri = 2 * ((size_t)(y / B) * Q + (size_t)(x / B)) + (a + b > P ? 1 : 0);
      const unsigned char* got = &t.atlas[((size_t)y * side + x) * 3];
      if (tri >= t.triangles()) {
        ++padding;
        wrong += got[0] != 0 || got[1] != 0 || got[2] != 0;
      } else {
        const unsigned char want = t.view[tri] < 0 ? 128 : shade[t.view[tri]];
        wrong += got[0] != want || got[1] != want || got[2] != want;
        wrong += (t.view[tri] >= 0) != (t.score[tri] > 0.0);
      }
    }
  ok = ok && wrong == 0 && padding > 0;
  for (size_t i = 0; ok && i < t.uv.size(); ++i) {
    const double texel = t.uv[i] * side - 0.5;
    ok = std::fabs(texel - std::floor(texel + 0.5)) < 1e-9 && texel > -0.5 && texel < side - 0.5;
  }

  double ms[4];
  long long launches[4];
  vol.getTextureProfile(ms, launches);
  std::printf("project %.3f, select %.3f, fill %.3f, fallback %.3f ms\n", ms[0], ms[1], ms[2], ms[3]);
  ok = ok && launches[0] == 2 && launches[1] == 2 && launches[2] == 2 && launches[3] == 1;
  const Mesh after = vol.simplified();
  ok = ok && after.xyz == coarse.xyz && after.faces == coarse.faces && after.grey == coarse.grey;            // the source stays

  const char* path = argc > 1 ? argv[1] : "atlas.ppm";
  FILE* f = std::fopen(path, "wb");
  if (!f) return 2;
  std::fprintf(f, "P6\n%d %d\n255\n", t.side, t.side);
  std::vector<unsigned char> rgb(t.atlas.size());
  for (size_t i = 0; i + 2 < rgb.size(); i += 3) {           // B, G, R -> R, G, B
    rgb[i] = t.atlas[i + 2]; rgb[i + 1] = t.atlas[i + 1]; rgb[i + 2] = t.atlas[i];
  }
  ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size() && ok;
  std::fclose(f);
  if (!ok) {
    std::printf("FAILED\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
