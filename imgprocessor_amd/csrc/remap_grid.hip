// remap_grid.hip — piecewise perspective-warp kernels (PerspectiveCorrection.correctGrid,
// camera/PerspectiveCorrection.py:281-372: one cv2.warpPerspective per lattice cell into views of
// one output array) as ONE launch of the gather kernel, and the plans behind it.
#include <vector>

#include "remap_impl.hpp"

extern "C" {

// Who owns which pixel.  The rectangles come in paint order and may overlap: the last one that
// covers a pixel owns it, as in a sequence of writes.  The output is cut at every rectangle edge
// into column bands and row bands (a rectangle is then a block of whole band pairs), and the
// rectangles are painted in order into the small band-pair matrix instead of the pixels:
// memory O(dh + dw + bands^2), no per-pixel cell map.
int ipa_warp_grid_plan(const int* cell_rects, int n_cells, int dh, int dw, uint16_t* colband,
                       uint16_t* rowband, int16_t* owner, int* n_rowbands, int* n_colbands) {
  IPA_REQUIRE(nullptr, cell_rects && n_rowbands && n_colbands, "warp_grid: null pointer");
  IPA_REQUIRE(nullptr, dh > 0 && dw > 0, "warp_grid: empty destination (%dx%d)", dh, dw);
  IPA_REQUIRE(nullptr, n_cells >= 1 && n_cells <= 32767, "warp_grid: n_cells must be in [1,32767] (got %d)",
              n_cells);
  std::vector<char> cutx((size_t)dw + 1, 0), cuty((size_t)dh + 1, 0);
  for (int i = 0; i < n_cells; i++) {
    const int x0 = cell_rects[4 * i], y0 = cell_rects[4 * i + 1], w = cell_rects[4 * i + 2],
              h = cell_rects[4 * i + 3];
    IPA_REQUIRE(nullptr, w > 0 && h > 0, "warp_grid: cell %d has an empty rectangle (%dx%d)", i, h, w);
    IPA_REQUIRE(nullptr, x0 >= 0 && y0 >= 0 && (long)x0 + w <= dw && (long)y0 + h <= dh,
                "warp_grid: rectangle of cell %d (x %d, y %d, %dx%d) is not inside the %dx%d destination", i, x0,
                y0, h, w, dh, dw);
    cutx[x0] = cutx[x0 + w] = 1;
    cuty[y0] = cuty[y0 + h] = 1;
  }
  // the band of a pixel: the number of edges in (0, pixel]
  long ncb = 1, nrb = 1;
  for (int x = 1; x < dw; x++) ncb += cutx[x];
  for (int y = 1; y < dh; y++) nrb += cuty[y];
  IPA_REQUIRE(nullptr, ncb <= 65535 && nrb <= 65535, "warp_grid: more than 65535 bands on an axis (%ld x %ld)",
              nrb, ncb);
  *n_colbands = (int)ncb;
  *n_rowbands = (int)nrb;
  std::vector<uint16_t> col((size_t)dw), row((size_t)dh);
  unsigned b = 0;
  for (int x = 0; x < dw; x++) col[x] = (uint16_t)(b += (x > 0 && cutx[x]) ? 1u : 0u);
  b = 0;
  for (int y = 0; y < dh; y++) row[y] = (uint16_t)(b += (y > 0 && cuty[y]) ? 1u : 0u);
  if (colband) memcpy(colband, col.data(), (size_t)dw * sizeof(uint16_t));
  if (rowband) memcpy(rowband, row.data(), (size_t)dh * sizeof(uint16_t));
  if (owner) {
    for (long i = 0; i < nrb * ncb; i++) owner[i] = -1;
    for (int i = 0; i < n_cells; i++) {
      const int x0 = cell_rects[4 * i], y0 = cell_rects[4 * i + 1], w = cell_rects[4 * i + 2],
                h = cell_rects[4 * i + 3];
      for (long r = row[y0]; r <= row[y0 + h - 1]; r++)
        for (long c = col[x0]; c <= col[x0 + w - 1]; c++) owner[r * ncb + c] = (int16_t)i;
    }
  }
  return IPA_OK;
}

}  // extern "C"

// the plan of (cells, dh, dw): from the context's cache, or made - with ipa_warp_grid_plan - and
// uploaded before this returns.  A plan's tables are never written again; the slot that makes way
// is freed only after the stream has drained (earlier launches may still read it).  The upload
// comes out of a buffer of this call's own: nothing an earlier asynchronous copy could still read.
static int grid_plan_get(ipa_ctx* ctx, const int* rects, const double* M, int n, int dh, int dw, GridCoord* gc) {
  IPA_REQUIRE(ctx, rects && M, "warp_grid: null cell_rects / cell_M");
  IPA_REQUIRE(ctx, n >= 1 && n <= 32767, "warp_grid: n_cells must be in [1,32767] (got %d)", n);
  const int head[3] = {dh, dw, n};
  const size_t rb = (size_t)n * 4 * sizeof(int), mb = (size_t)n * 9 * sizeof(double);
  std::vector<char> key(sizeof head + rb + mb);
  memcpy(key.data(), head, sizeof head);
  memcpy(key.data() + sizeof head, rects, rb);
  memcpy(key.data() + sizeof head + rb, M, mb);
  ipa_ctx::GridPlan* pl = nullptr;
  for (auto& q : ctx->grid_plans)
    if (q.dev && q.key.size() == key.size() && memcmp(q.key.data(), key.data(), key.size()) == 0) pl = &q;
  if (!pl) {
    int nrb = 0, ncb = 0;
    int rc = ipa_warp_grid_plan(rects, n, dh, dw, nullptr, nullptr, nullptr, &nrb, &ncb);   // validates, counts
    if (rc) {
      ctx->last_error = ipa_last_error(nullptr);
      return rc;
    }
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t off_owner = up((size_t)n * sizeof(GridCell));
    const size_t off_col = off_owner + up((size_t)nrb * ncb * sizeof(int16_t));
    const size_t off_row = off_col + up((size_t)dw * sizeof(uint16_t));
    const size_t total = off_row + up((size_t)dh * sizeof(uint16_t));
    std::vector<char> blob(total, 0);
    rc = ipa_warp_grid_plan(rects, n, dh, dw, reinterpret_cast<uint16_t*>(blob.data() + off_col),
                            reinterpret_cast<uint16_t*>(blob.data() + off_row),
                            reinterpret_cast<int16_t*>(blob.data() + off_owner), &nrb, &ncb);
    if (rc) {
      ctx->last_error = ipa_last_error(nullptr);
      return rc;
    }
    GridCell* cells = reinterpret_cast<GridCell*>(blob.data());
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < 9; k++) cells[i].m[k] = M[9 * i + k];
      cells[i].x0 = rects[4 * i];
      cells[i].y0 = rects[4 * i + 1];
    }
    pl = &ctx->grid_plans[0];
    for (auto& q : ctx->grid_plans)
      if (!q.dev || q.used < pl->used) { pl = &q; if (!q.dev) break; }
    IPA_HIP(ctx, hipSetDevice(ctx->device));
    if (pl->dev) {
      IPA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      void* old = pl->dev;
      pl->dev = nullptr;
      pl->key.clear();
      IPA_HIP(ctx, hipFree(old));
    }
    void* dev = nullptr;
    IPA_HIP(ctx, hipMalloc(&dev, total));
    hipError_t e = hipMemcpyAsync(dev, blob.data(), total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // `blob` dies with this call
    if (e != hipSuccess) {
      (void)hipFree(dev);
      IPA_HIP(ctx, e);
    }
    pl->dev = dev;
    pl->key.swap(key);
    pl->off_owner = off_owner;
    pl->off_col = off_col;
    pl->off_row = off_row;
    pl->n_colbands = ncb;
  }
  pl->used = ++ctx->grid_plan_clock;
  const char* d = static_cast<const char*>(pl->dev);
  gc->cells = reinterpret_cast<const GridCell*>(d);
  gc->owner = reinterpret_cast<const int16_t*>(d + pl->off_owner);
  gc->colband = reinterpret_cast<const uint16_t*>(d + pl->off_col);
  gc->rowband = reinterpret_cast<const uint16_t*>(d + pl->off_row);
  gc->n_colbands = pl->n_colbands;
  return IPA_OK;
}

int ipa_remap_launch_grid(ipa_ctx* ctx, const RemapCall& a, const int* cell_rects, const double* cell_M,
                          int n_cells) {
  if (!ctx) return IPA_ERR_BAD_ARG;
  IPA_REQUIRE(ctx, a.dh > 0 && a.dw > 0, "empty image (%dx%d -> %dx%d)", a.sh, a.sw, a.dh, a.dw);
  GridCoord c;
  int rc = grid_plan_get(ctx, cell_rects, cell_M, n_cells, a.dh, a.dw, &c);
  if (rc) return rc;
  return remap_dispatch<GridCoord>(ctx, a, c, 0);
}
