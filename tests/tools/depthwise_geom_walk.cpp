// Host walk of the launch geometry of csrc/depthwise.hip: includes csrc/depthwise_geom.h, the header the kernels' file includes, and forms, for
// every shape on the command line and both paths (V = 1, and V = 4 where the channel count allows it), every index the three kernels form --
// block by block and thread by thread, with the kernels' own loops -- inside host buffers of the stated sizes.  Every output element and every
// partial sum of the workspace must be written exactly once.  Built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_sepconv_cpu.py); an index outside a buffer is the sanitizer's report, a wrong count is exit status 1.
//
// arguments: groups of nine integers  B L C k stride dilation dm pad_left Lout
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "depthwise_geom.h"

using namespace gn;
typedef unsigned long long ull;

struct Shape {
  int B, L, C, k, s, d, dm, pl, Lout, CO;
};

static int fail(const char* what, const Shape& g, int V) {
  std::printf("FAILED %s: B %d L %d C %d k %d s %d d %d dm %d pl %d Lout %d V %d\n", what, g.B, g.L, g.C, g.k, g.s, g.d, g.dm, g.pl, g.Lout, V);
  return 1;
}

static bool all_one(const std::vector<unsigned char>& n) {
  for (unsigned char v : n)
    if (v != 1) return false;
  return true;
}

// touch V consecutive floats (a 16-byte access on the vector path)
static void touch(const std::vector<float>& a, ull i, int V, float* sink) {
  for (int j = 0; j < V; ++j) *sink += a[i + j];
}

static int walk(const Shape& g, int V) {
  const std::vector<float> x((size_t)g.B * g.L * g.C, 1.f), w((size_t)g.k * g.CO, 1.f), dy((size_t)g.B * g.Lout * g.CO, 1.f);
  float sink = 0.f;
  const bool dm1 = g.dm == 1, dm2v = g.dm == 2 && V == DW_VEC;       // the 16-byte form, the 8-byte pair of x under dm == 2

  {  // forward
    std::vector<unsigned char> y((size_t)g.B * g.Lout * g.CO, 0);
    const ull nvec = g.CO / V;
    const int RS = dw_fwd_row_lanes((long long)nvec, g.Lout);
    const ull lgroups = (g.Lout + DW_ROWS * RS - 1) / (DW_ROWS * RS), items = (ull)g.B * lgroups * RS * nvec;
    if (RS < 1 || (RS > 1 && (ull)RS * nvec > (ull)DW_WAVE)) return fail("forward row lanes", g, V);
    if (items != dw_fwd_items(g.B, g.Lout, g.C, g.dm, V)) return fail("forward items", g, V);
    const unsigned grid = dw_stream_grid(items);
    if (grid < 1 || grid > (unsigned)DW_GRID_CAP) return fail("forward grid", g, V);
    for (unsigned blk = 0; blk < grid; ++blk)
      for (int tid = 0; tid < DW_BLOCK; ++tid)
        for (ull item = (ull)blk * DW_BLOCK + tid; item < items; item += (ull)grid * DW_BLOCK) {
          const int co = (int)(item % nvec) * V;
          ull rest = item / nvec;
          const int rs = (int)(rest % RS);
          rest /= RS;
          const int l0 = (int)(rest % lgroups) * DW_ROWS * RS + rs;
          const ull b = rest / lgroups;
          for (int t = 0; t < g.k; ++t) {
            touch(w, (ull)t * g.CO + co, V, &sink);
            for (int r = 0; r < DW_ROWS; ++r) {
              const long long p = dw_in_row(l0 + r * RS, g.s, g.pl, t, g.d);
              if (l0 + r * RS < g.Lout && p >= 0 && p < g.L) {
                const ull row = (b * g.L + p) * g.C;
                if (dm1) touch(x, row + co, V, &sink);
                else if (dm2v) touch(x, row + co / 2, 2, &sink);
                else
                  for (int j = 0; j < V; ++j) touch(x, row + (co + j) / g.dm, 1, &sink);
              }
            }
          }
          for (int r = 0; r < DW_ROWS; ++r)
            if (l0 + r * RS < g.Lout)
              for (int j = 0; j < V; ++j) ++y[(b * g.Lout + l0 + r * RS) * g.CO + co + j];
        }
    if (!all_one(y)) return fail("forward: an output not written exactly once", g, V);
  }

  if (g.C % V == 0) {  // data gradient
    std::vector<unsigned char> dx((size_t)g.B * g.L * g.C, 0);
    const ull nvec = g.C / V, items = (ull)g.B * g.L * nvec;
    if (items != dw_dgrad_items(g.B, g.L, g.C, V)) return fail("data gradient items", g, V);
    const unsigned grid = dw_stream_grid(items);
    for (unsigned blk = 0; blk < grid; ++blk)
      for (int tid = 0; tid < DW_BLOCK; ++tid)
        for (ull item = (ull)blk * DW_BLOCK + tid; item < items; item += (ull)grid * DW_BLOCK) {
          const int c = (int)(item % nvec) * V;
          const ull rest = item / nvec;
          const int i = (int)(rest % g.L);
          const ull b = rest / g.L;
          for (int t = 0; t < g.k; ++t) {
            const long long num = (long long)i + g.pl - (long long)t * g.d;
            if (num < 0) break;
            if (num % g.s) continue;
            const long long l = num / g.s;
            if (l >= g.Lout) continue;
            if (dw_in_row(l, g.s, g.pl, t, g.d) != i) return fail("data gradient: the gathered row does not read this input row", g, V);
            const ull row = (b * g.Lout + l) * g.CO;
            if (dm1) {
              touch(dy, row + c, V, &sink);
              touch(w, (ull)t * g.CO + c, V, &sink);
            } else if (dm2v) {
              for (int h = 0; h < 2; ++h) {
                touch(dy, row + 2 * (ull)c + 4 * h, 4, &sink);
                touch(w, (ull)t * g.CO + 2 * (ull)c + 4 * h, 4, &sink);
              }
            } else {
              for (int j = 0; j < V; ++j)
                for (int m = 0; m < g.dm; ++m) {
                  touch(dy, row + (ull)(c + j) * g.dm + m, 1, &sink);
                  touch(w, (ull)t * g.CO + (ull)(c + j) * g.dm + m, 1, &sink);
                }
            }
          }
          for (int j = 0; j < V; ++j) ++dx[(b * g.L + i) * g.C + c + j];
        }
    if (!all_one(dx)) return fail("data gradient: an output not written exactly once", g, V);
  }

  {  // weight gradient
    const DwWgradGeom m = dw_wgrad_geom(g.B, g.Lout, g.C, g.k, g.dm, V);
    const size_t n = (size_t)g.k * g.CO;
    if (m.ws_bytes != dw_wgrad_geom(g.B, g.Lout, g.C, g.k, g.dm, 1).ws_bytes || m.ws_bytes != (size_t)m.parts * n * sizeof(double))
      return fail("weight gradient: the workspace depends on the path", g, V);
    if (m.parts < 1 || m.parts > DW_WG_MAX_PARTS || m.rpp * (ull)m.parts < m.rows || m.rpp * (ull)(m.parts - 1) >= m.rows)
      return fail("weight gradient: an empty part, or rows outside every part", g, V);
    if (m.NC < 1 || m.RL < 1 || m.NC * m.RL > DW_BLOCK || (long long)m.ctiles * m.NC < (long long)g.CO / V)
      return fail("weight gradient: the lanes of a block", g, V);
    std::vector<unsigned char> part(m.ws_bytes / sizeof(double), 0), rows_seen(m.rows * (size_t)(g.CO / V), 0);
    std::vector<float> red((size_t)DW_WG_TAPS * V * DW_BLOCK, 0.f);
    const long long nvec = g.CO / V;
    for (int by = 0; by < m.parts; ++by)
      for (int bx = 0; bx < m.ctiles; ++bx) {
        const ull r0 = (ull)by * m.rpp, r1 = r0 + m.rpp < m.rows ? r0 + m.rpp : m.rows;
        for (int t0 = 0; t0 < g.k; t0 += DW_WG_TAPS) {
          for (int tid = 0; tid < DW_BLOCK; ++tid) {
            const int cl = tid % m.NC, rl = tid / m.NC;
            const long long cv = (long long)bx * m.NC + cl;
            const bool active = rl < m.RL && cv < nvec;
            const int co = active ? (int)cv * V : 0;
            if (active)
              for (ull r = r0 + rl; r < r1; r += m.RL) {
                const ull b = r / g.Lout;
                const long long l = (long long)(r - b * g.Lout);
                touch(dy, r * g.CO + co, V, &sink);
                if (t0 == 0) ++rows_seen[r * nvec + cv];
                for (int tt = 0; tt < DW_WG_TAPS; ++tt) {
                  const long long p = dw_in_row(l, g.s, g.pl, t0 + tt, g.d);
                  if (t0 + tt < g.k && p >= 0 && p < g.L) {
                    const ull row = (b * g.L + p) * g.C;
                    if (dm1) touch(x, row + co, V, &sink);
                    else if (dm2v) touch(x, row + co / 2, 2, &sink);
                    else
                      for (int j = 0; j < V; ++j) touch(x, row + (co + j) / g.dm, 1, &sink);
                  }
                }
              }
            for (int tj = 0; tj < DW_WG_TAPS * V; ++tj) red[(size_t)tj * DW_BLOCK + tid] = 1.f;
          }
          for (int tid = 0; tid < DW_BLOCK; ++tid)
            for (int o = tid; o < DW_WG_TAPS * V * m.NC; o += DW_BLOCK) {
              const int tj = o / m.NC, c2 = o % m.NC, t = t0 + tj / V;
              const long long cv2 = (long long)bx * m.NC + c2;
              if (t < g.k && cv2 < nvec) {
                for (int q = 0; q < m.RL; ++q) {
                  if (q * m.NC + c2 >= DW_BLOCK) return fail("weight gradient: a row lane outside the block", g, V);
                  sink += red[(size_t)tj * DW_BLOCK + q * m.NC + c2];
                }
                ++part[(size_t)by * n + (size_t)t * g.CO + (size_t)cv2 * V + tj % V];
              }
            }
        }
      }
    if (!all_one(part)) return fail("weight gradient: a partial sum not written exactly once", g, V);
    if (!all_one(rows_seen)) return fail("weight gradient: a row not summed exactly once", g, V);
  }
  return sink < 0.f;       // never: keeps the reads
}

int main(int argc, char** argv) {
  if (argc < 10 || (argc - 1) % 9) {
    std::printf("usage: depthwise_geom_walk  B L C k stride dilation dm pad_left Lout  [nine more ...]\n");
    return 2;
  }
  int walked = 0;
  for (int a = 1; a + 8 < argc; a += 9) {
    Shape g;
    int* f[9] = {&g.B, &g.L, &g.C, &g.k, &g.s, &g.d, &g.dm, &g.pl, &g.Lout};
    for (int i = 0; i < 9; ++i) *f[i] = std::atoi(argv[a + i]);
    g.CO = g.C * g.dm;
    if (walk(g, 1)) return 1;
    ++walked;
    if (g.CO % DW_VEC == 0) {
      if (walk(g, DW_VEC)) return 1;
      ++walked;
    }
  }
  std::printf("walked %d launches of each kernel\n", walked);
  return 0;
}
