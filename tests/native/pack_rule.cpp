// The cells-per-lane rule of the record units (csrc/mlx_record.hpp: pack_width) against its
// statement, exhaustively over small shapes, and the three operand shapes that the units used to
// spell by hand.  Host code only: no HIP call is made.
//
// Rule A: take the widest v in {16 / elem, .., 2, 1} such that n % v == 0 and every operand's row
// start is aligned to min(16, bytes_per_cell * v); a NULL operand is skipped.  An operand that is
// not aligned to its own cell satisfies no v -- the entry points refuse it before they ask -- and
// pack_width then answers 1.
#include <cstdint>
#include <cstdio>

#include "../../momlevel_amd/csrc/mlx_record.hpp"

namespace {

struct Op {
  uintptr_t p;
  size_t cell;
};

int rule_a(int64_t n, size_t elem, const Op* ops, int nops) {
  for (int v = (int)(16 / elem); v >= 1; v /= 2) {
    if (n % v != 0) continue;
    bool ok = true;
    for (int i = 0; i < nops; ++i) {
      if (ops[i].p == 0) continue;
      const size_t access = ops[i].cell * v < 16 ? ops[i].cell * v : 16;
      if (ops[i].p % access != 0) ok = false;
    }
    if (ok) return v;
  }
  return 1;
}

const void* ptr(uintptr_t p) { return reinterpret_cast<const void*>(p); }

int failures = 0;

void expect(int got, int want, const char* what) {
  if (got == want) return;
  std::printf("FAIL %s: pack_width %d, expected %d\n", what, got, want);
  ++failures;
}

}  // namespace

int main() {
  long cases = 0;
  for (size_t elem : {(size_t)4, (size_t)8})
    for (int64_t n = 1; n <= 17; ++n)
      for (size_t c0 : {(size_t)4, (size_t)8})
        for (size_t c1 : {(size_t)4, (size_t)8})
          for (uintptr_t p0 = 0; p0 < 32; p0 += 4)
            for (uintptr_t p1 = 0; p1 < 32; p1 += 4) {
              const Op ops[2] = {{p0, c0}, {p1, c1}};
              const int want = rule_a(n, elem, ops, 2);
              const int got = mlx::pack_width(n, elem, {{ptr(p0), c0}, {ptr(p1), c1}});
              ++cases;
              if (got != want) {
                std::printf("FAIL elem %zu n %lld operands (%zu @ %zu) (%zu @ %zu): pack_width %d, "
                            "expected %d\n", elem, (long long)n, (size_t)p0, c0, (size_t)p1, c1, got, want);
                ++failures;
              }
            }

  const uintptr_t base = 1 << 20;  // 16-byte aligned
  // the fits: the float32 record at elem * v, the float64 workspace at 8 * (v > 2 ? 2 : v)
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base), 8}}), 4, "fit, all aligned");
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base + 8), 8}}), 1, "fit, workspace 8 off");
  expect(mlx::pack_width(8, 4, {{ptr(base + 8), 4}, {ptr(base), 8}}), 2, "fit, record 8 off");
  expect(mlx::pack_width(8, 8, {{ptr(base), 8}, {ptr(base + 8), 8}}), 1, "fit float64, workspace 8 off");
  expect(mlx::pack_width(8, 8, {{nullptr, 8}, {ptr(base), 8}}), 2, "apply, y not read");
  expect(mlx::pack_width(6, 4, {{ptr(base), 4}, {ptr(base), 8}}), 2, "fit, n % 4 == 2");
  // the exceedance count: thr and out are 8-byte cells, 16-byte accesses for v >= 2
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base), 8}, {ptr(base), 8}}), 4, "exceed, all aligned");
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base + 8), 8}, {ptr(base), 8}}), 1, "exceed, thr 8 off");
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base), 8}, {ptr(base + 8), 8}}), 1, "exceed, out 8 off");
  expect(mlx::pack_width(8, 4, {{ptr(base + 8), 4}, {ptr(base), 8}, {ptr(base), 8}}), 2, "exceed, y 8 off");
  // the filter: float32 in, float64 out -- a 32-byte result pack moves as two accesses of 16
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base), 8}}), 4, "filter f32->f64, all aligned");
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base + 8), 8}}), 1, "filter f32->f64, out 8 off");
  expect(mlx::pack_width(8, 8, {{ptr(base), 8}, {ptr(base + 8), 4}}), 2, "filter f64->f32, out 8 off");
  expect(mlx::pack_width(8, 8, {{ptr(base), 8}, {ptr(base + 4), 4}}), 1, "filter f64->f32, out 4 off");
  expect(mlx::pack_width(8, 4, {{ptr(base), 4}, {ptr(base + 8), 4}}), 2, "filter f32->f32, out 8 off");

  if (failures) {
    std::printf("pack_rule: %d failures in %ld cases\n", failures, cases);
    return 1;
  }
  std::printf("pack_rule OK (%ld cases)\n", cases);
  return 0;
}
