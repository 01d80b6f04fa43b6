// Host check of the loss workspaces (csrc/bts_host.h: Carver; tiled_layout, median_layout, pixel_layout): the counted size is where the carved pointers end.
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/loss_workspace_check.hip -o /tmp/loss_workspace_check
//   /tmp/loss_workspace_check          (launches nothing: needs no GPU)
// The two .hip files are compiled INTO this program, so it calls the layout functions the library calls (they live in the files'
// anonymous namespaces).
#include "../behindthescenes_amd/csrc/bts_loss_tiled.hip"
#include "../behindthescenes_amd/csrc/bts_loss_pixel.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bts {
void set_error(const char*, const char*, long, long, long) {}      // bts_fwd.hip's, not linked here

// [first, last + last_bytes) must be exactly the `bytes - 256` behind the rounded-up workspace pointer, inside the allocation
static int check(const char* what, const char* ws, const char* alloc_end, size_t bytes, const void* first, const void* last, size_t last_bytes,
                 const int* shape) {
  const char* base = reinterpret_cast<const char*>(up256((size_t)(uintptr_t)ws));
  const char* end = reinterpret_cast<const char*>(last) + up256(last_bytes);
  const bool ok = first == base && end == base + (bytes - kAlign) && end <= alloc_end;
  if (ok) memset(const_cast<char*>(base), 0x5a, (size_t)(end - base));      // every byte handed out is the caller's
  printf("%-22s (%d, %d, %d, %d): %zu bytes %s\n", what, shape[0], shape[1], shape[2], shape[3], bytes, ok ? "ok" : "MISMATCH");
  return ok ? 0 : 1;
}
}  // namespace bts

int main() {
  using namespace bts;
  static const int shapes[5][4] = {{1, 1, 1, 1}, {3, 8, 8, 2}, {2, 16, 16, 1}, {2, 17, 33, 4}, {1, 192, 640, 1}};   // n_patches, ph, pw, nv
  int bad = 0;
  for (const int* s : shapes) {
    const size_t B = (size_t)s[0] * s[1] * s[2], nt = (size_t)s[0] * (size_t)tiles_of(s[1], s[2]);
    for (int thr = 0; thr < 2; ++thr) {
      const size_t bytes = loss_tiled_bytes(s[0], s[1], s[2], s[3], thr != 0);
      char* ws = static_cast<char*>(malloc(bytes));
      char* given = ws + thr;      // once as malloc aligned it, once off by one byte
      Carver carve(given);
      TiledParamsThr p;
      tiled_layout(carve, p, (size_t)s[0], nt, B, thr != 0);
      bad += carve.bytes() != bytes;
      bad += thr ? check("tiled, automask", given, ws + bytes, bytes, p.tile_parts, p.fthr, B * sizeof(float), s)
                 : check("tiled", given, ws + bytes, bytes, p.tile_parts, p.keep, B, s);
      free(ws);
    }
    for (int n = 1; n <= 2; ++n) {
      if (s[0] % n) continue;
      const size_t bytes = loss_median_bytes(s[0], s[1], s[2], s[3], n);
      char* ws = static_cast<char*>(malloc(bytes));
      char* given = ws + (n - 1);      // once as malloc aligned it, once off by one byte
      Carver carve(given);
      TiledParamsMed p;
      median_layout(carve, p, (size_t)s[0], nt, B, (size_t)n, (size_t)n * median_blocks_per_sample((size_t)s[0], (size_t)n, s[1], s[2]));
      bad += carve.bytes() != bytes;
      const int shape[4] = {s[0], s[1], s[2], n};
      bad += check("tiled, median (.., n)", given, ws + bytes, bytes, p.tile_parts, p.fin, 4 * sizeof(float), shape);
      free(ws);
    }
    for (int n = 1; n <= 2; ++n) {
      const size_t bytes = pixel_loss_bytes((long)B, n, s[1], s[2]);
      char* ws = static_cast<char*>(malloc(bytes));
      Carver carve(ws);
      PixelParams p;
      pixel_layout(carve, p, B, (size_t)n, geom_of((long)B, n, s[1], s[2]));
      bad += carve.bytes() != bytes;
      const int shape[4] = {s[0], s[1], s[2], n};
      bad += check("pixel (.., n)", ws, ws + bytes, bytes, p.e, p.fin, 4 * sizeof(float), shape);
      free(ws);
    }
  }
  printf(bad ? "FAILED\n" : "all layouts end where their size says\n");
  return bad ? 1 : 0;
}
