// The textured test sphere seen through include/vslam_filter_hip.hpp's TsdfVolumeHip::rasterise.  The
// volume is written directly: the analytic sphere of radius 1.25 round the world origin on a 17 x 15 x 13 grid.  The demo welds,
// textures the weld at a patch of 4 texels from two views of constant grey (one on the -z axis, one on the +z axis), rasterises
// it from the first view's pose with the atlas, with cover, and holds a few invariants: every hit pixel is covered, without
// culling by at least one triangle more, its depth lies between the camera's distance to the sphere and to its centre, a pixel
// of a triangle the first view textured carries exactly that view's constant and one of a triangle without a view the blend of
// its vertices' grey (128 everywhere), a pixel without a hit is all zero, the weld given back through setRasterMesh shows the same triangles at the same
// depths, the result does not depend on small_limit, and the weld is what it was.  It writes the Lambert-shaded colour image as
// raster.ppm (or the path given).  Prints "ok" on success.
#include <cmath>
#include <cstdio>
#include <vector>

#include "vslam_filter_hip.hpp"

typedef TsdfVolumeHip::IndexedMesh Mesh;
typedef TsdfVolumeHip::MeshRender Image;

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

  const Mesh weld = vol.weld(1);
  const int W = 64, H = 48;
  const double K[4] = {60.0, 60.0, 31.5, 23.5};
  const double front[7] = {0.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0}, back[7] = {0.0, 0.0, 4.0, 0.0, 0.0, 1.0, 0.0};   // half a turn about y
  const unsigned char shade[2] = {80, 200};
  vol.textureBegin(0, 4, 3);                                // 3 channels over a plain volume: grey, replicated
  for (int v = 0; v < 2; ++v) {
    const std::vector<unsigned char> img((size_t)W * H, shade[v]);
    vol.textureAddViewHost(img.data(), 1, W, H, K, v ? back : front);
  }
  const TsdfVolumeHip::TextureAtlas atlas = vol.textureFinish();

  vol.profile(true);
  const Image r = vol.rasterise(W, H, K, front, 0, 0.0, true, 1, true);
  bool ok = r.width == W && r.height == H && r.colour.size() == (size_t)W * H * 3 && r.cover.size() == (size_t)W * H;
  size_t hit = 0, textured = 0, wrong = 0;
  for (size_t p = 0; ok && p < (size_t)W * H; ++p) {
    const unsigned char* c = &r.colour[p * 3];
    if (r.tri[p] < 0) {
      wrong += r.depth[p] != 0.f || r.cover[p] != 0 || r.grey[p] != 0 || c[0] != 0 || c[1] != 0 || c[2] != 0 || r.normal[p * 3 + 2] != 0.f;
      continue;
    }
    ++hit;
    const int view = atlas.view[(size_t)r.tri[p]];
    const unsigned char want = view < 0 ? 128 : shade[view];
    textured += view == 0;
    wrong += (size_t)r.tri[p] >= weld.triangles() || r.cover[p] < 1 || !(r.depth[p] > 4.0f - 1.26f && r.depth[p] < 4.0f);
    wrong += view == 1 || c[0] != want || c[1] != want || c[2] != want || r.grey[p] != want;
    wrong += !(r.normal[p * 3 + 2] < 0.f);                   // the weld's triangles face free space: towards the camera
  }
  ok = ok && wrong == 0 && hit > 500 && textured > hit / 2;
  std::printf("%zu triangles, %d x %d pixels, %zu hit, %zu of them textured by the first view\n", weld.triangles(), W, H, hit, textured);

  double ms[4];
  long long launches[4];
  vol.getRasterProfile(ms, launches);
  std::printf("project %.3f, small %.3f, large %.3f, resolve %.3f ms\n", ms[0], ms[1], ms[2], ms[3]);
  ok = ok && launches[0] == 1 && launches[1] == 1 && launches[2] == 1 && launches[3] == 1;

  // every triangle through the workgroup path, then none: the same images
  vol.setRasterSmallLimit(0);
  const Image all_large = vol.rasterise(W, H, K, front, 0, 0.0, true, 1, true);
  vol.setRasterSmallLimit(65536);
  const Image all_small = vol.rasterise(W, H, K, front, 0, 0.0, true, 1, true);
  vol.getRasterProfile(ms, launches);
  ok = ok && launches[1] == 3 && launches[2] == 2;          // 65536 >= 64 x 48: k_rast_large is not launched
  for (const Image* o : {&all_large, &all_small})
    ok = ok && o->depth == r.depth && o->tri == r.tri && o->bary == r.bary && o->colour == r.colour && o->cover == r.cover && o->normal == r.normal;
  vol.setRasterSmallLimit(16);

  // the weld given back by the caller, with its vertex colours, without culling: the same triangles in front
  vol.setRasterMesh(weld.xyz, weld.faces, weld.grey);
  const Image own = vol.rasterise(W, H, K, front, 4, 0.0, false, 0, true);
  ok = ok && own.colour.empty() && own.tri == r.tri && own.depth == r.depth;
  for (size_t p = 0; ok && p < (size_t)W * H; ++p) ok = (r.tri[p] < 0 ? own.cover[p] == 0 : own.cover[p] > r.cover[p]) && own.grey[p] == (r.tri[p] < 0 ? 0 : 128);
  const Mesh after = vol.mesh();
  ok = ok && after.xyz == weld.xyz && after.faces == weld.faces && after.grey == weld.grey;                  // the source stays

  const char* path = argc > 1 ? argv[1] : "raster.ppm";
  FILE* f = std::fopen(path, "wb");
  if (!f) return 2;
  std::fprintf(f, "P6\n%d %d\n255\n", W, H);
  std::vector<unsigned char> rgb((size_t)W * H * 3);
  for (size_t p = 0; p < (size_t)W * H; ++p) {              // Lambert, the light behind the camera; B, G, R -> R, G, B
    const double lam = std::max(0.0, -(double)r.normal[p * 3 + 2]);
    for (int ch = 0; ch < 3; ++ch) rgb[p * 3 + ch] = (unsigned char)std::floor(r.colour[p * 3 + 2 - ch] * lam + 0.5);
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
