// Stand-alone run of egnn_cell_relax_host and egnn_cell_relax_step_host (csrc/cells/cell_relax_host.cpp), built with
// -fsanitize=address,undefined by tests/test_cell_relax_host.py.  Every array has EXACTLY the size the contract states, so that ASan
// sees a write past a trace row, a force or a counter.  The program checks memory and argument handling; the trajectories are
// test_cell_relax_host.py's business.  Cases: displaced rocksalt (8 atoms, unlike-pair Born-Mayer repulsion) with a skin of 0.4 A,
// small enough that the list is rebuilt, alone and in a batch with a one-atom cell and an empty cell, with and without the
// traces; the same cell strongly compressed, where the cap is active at max_step == skin / 2; a cell with coincident atoms; the
// step alone on cells of 1, 257 and 0 atoms; every bad-argument case.
#include <math.h>
#include "../../include/egnn_amd.h"
#include "cell_fixtures.h"

using namespace cell_fixtures;

namespace {

struct Run {
  double f_max = 1e-6, skin = 0.4, max_step = 0.2, r_cut = 6.0, short_cut = 6.0, f_dec = 0.5;
  int max_steps = 480;
  bool traces = true;
};

struct Result {
  std::vector<double> frac, energy, initial, force, max_force, moved, e_trace, f_trace, x_trace;
  std::vector<int32_t> steps, status, rebuilds;
};

void add_rocksalt(Cells& b) {
  const double na[4][3] = {{0, 0, 0}, {0, .5, .5}, {.5, 0, .5}, {.5, .5, 0}};
  std::vector<double> f;
  std::vector<int32_t> t;
  for (int o = 0; o < 2; ++o)
    for (int k = 0; k < 4; ++k) {
      for (int x = 0; x < 3; ++x) f.push_back(na[k][x] + 0.5 * o + 0.013 + (0.3 * uniform() - 0.15) / 5.64);
      t.push_back(o);
    }
  b.add(5.64, f, t);
}

int call(const Cells& b, const Run& r, Result* out) {
  const size_t C = b.C(), N = b.N(), rows = (size_t)(r.max_steps < 0 ? 0 : r.max_steps) + 1;
  const double charges[2] = {1.0, -1.0};
  const double pot[16] = {0.0, 1200.0, 1200.0, 0.0, 1.0, 3.125, 3.125, 1.0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double alpha = sqrt(-log(1e-8)) / r.r_cut, k_max = 2.0 * alpha * sqrt(-log(1e-8));
  out->frac.assign(3 * N, -7.0);
  out->force.assign(3 * N, -7.0);
  out->moved.assign(3 * N, -7.0);
  out->energy.assign(C, -7.0);
  out->initial.assign(C, -7.0);
  out->max_force.assign(C, -7.0);
  out->steps.assign(C, -7);
  out->status.assign(C, -7);
  out->rebuilds.assign(C, -7);
  out->e_trace.assign(r.traces ? rows * C : 0, -7.0);
  out->f_trace.assign(r.traces ? rows * C : 0, -7.0);
  out->x_trace.assign(r.traces ? rows * 3 * N : 0, -7.0);
  return egnn_cell_relax_host(b.C(), 2, b.cell_ptr.data(), b.lattice.data(), b.frac.data(), b.type.data(), charges, pot, 24, 1, 14.3996454784,
                              alpha, r.r_cut, r.short_cut, k_max, 0.1, 1.0, 5, 1.1, r.f_dec, 0.1, 0.99, r.max_step, r.f_max, r.max_steps, r.skin,
                              out->frac.data(), out->energy.data(), out->initial.data(), out->force.data(), out->max_force.data(),
                              out->steps.data(), out->status.data(), out->moved.data(), out->rebuilds.data(),
                              r.traces ? out->e_trace.data() : nullptr, r.traces ? out->f_trace.data() : nullptr,
                              r.traces ? out->x_trace.data() : nullptr);
}

Result run(const Cells& b, const Run& r) {
  Result out;
  const int rc = call(b, r, &out);
  CHECK(rc == 0, "rc %d: %s", rc, egnn_last_error());
  for (const std::vector<double>* v : {&out.frac, &out.energy, &out.initial, &out.force, &out.max_force, &out.moved})
    for (double x : *v) CHECK(isfinite(x) && x != -7.0, "an output was not written");
  for (const std::vector<double>* v : {&out.e_trace, &out.f_trace, &out.x_trace})
    for (double x : *v) CHECK(x != -7.0, "a trace entry was not written");
  for (size_t c = 0; c < out.steps.size(); ++c) CHECK(out.steps[c] >= 0 && out.status[c] >= 1 && out.status[c] <= 5 && out.rebuilds[c] >= 0, "cell %zu", c);
  return out;
}

}  // namespace

int main() {
  seed(24680);
  Cells salt, mixed;
  add_rocksalt(salt);
  mixed.add(5.0, {0.1, 0.2, 0.3}, {0});
  mixed.lattice.insert(mixed.lattice.end(), salt.lattice.begin(), salt.lattice.end());
  mixed.frac.insert(mixed.frac.end(), salt.frac.begin(), salt.frac.end());
  mixed.type.insert(mixed.type.end(), salt.type.begin(), salt.type.end());
  mixed.cell_ptr.push_back(mixed.N());
  mixed.add(5.0, {}, {});   // an empty cell: converged at once
  {
    const Result alone = run(salt, Run());
    CHECK(alone.status[0] == 1 && alone.steps[0] > 10 && alone.steps[0] <= 480, "rocksalt: status %d after %d moves", alone.status[0], alone.steps[0]);
    CHECK(alone.rebuilds[0] >= 1, "the skin of 0.4 A must force a rebuild (%d)", alone.rebuilds[0]);
    CHECK(alone.max_force[0] < 1e-6 && alone.energy[0] < alone.initial[0], "rocksalt: max |F| %g", alone.max_force[0]);
    CHECK(alone.e_trace[0] == alone.initial[0] && alone.e_trace[alone.steps[0]] == alone.energy[0], "the trace");
    CHECK(alone.steps[0] == 480 || isnan(alone.e_trace[alone.steps[0] + 1]), "the trace beyond the last evaluation");
    Run bare;
    bare.traces = false;
    const Result quiet = run(salt, bare), batch = run(mixed, Run());
    for (size_t k = 0; k < alone.frac.size(); ++k) {
      CHECK(quiet.frac[k] == alone.frac[k], "the traces change coordinate %zu", k);
      CHECK(batch.frac[3 + k] == alone.frac[k] && batch.moved[3 + k] == alone.moved[k], "coordinate %zu differs in the batch", k);
    }
    CHECK(batch.energy[1] == alone.energy[0] && batch.steps[1] == alone.steps[0] && batch.rebuilds[1] == alone.rebuilds[0], "the batch");
    CHECK(batch.status[0] == 1 && batch.steps[0] == 0 && batch.status[2] == 1 && batch.steps[2] == 0, "the one-atom and the empty cell");
    Run few;
    few.max_steps = 7;
    const Result cut = run(salt, few);
    CHECK(cut.status[0] == 2 && cut.steps[0] == 7, "the step limit: status %d after %d", cut.status[0], cut.steps[0]);
    few.max_steps = 0;
    const Result none = run(salt, few);
    CHECK(none.status[0] == 2 && none.steps[0] == 0 && none.energy[0] == none.initial[0], "max_steps = 0");
  }
  {   // a strongly compressed cell at max_step == skin / 2: the cap is active when the cell freezes, and it must move after the rebuild
    seed(97531);
    Cells tight;
    add_rocksalt(tight);
    for (int k = 0; k < 9; ++k) tight.lattice[k] *= 3.8 / 5.64;
    Run r;
    r.f_max = 1e-4;
    r.max_steps = 600;
    const Result out = run(tight, r);
    CHECK(out.status[0] == 1 || out.status[0] == 2, "the compressed cell: status %d", out.status[0]);
    CHECK(out.rebuilds[0] >= 1 && out.rebuilds[0] <= out.steps[0], "the compressed cell: %d rebuilds in %d moves", out.rebuilds[0], out.steps[0]);
  }
  {   // coincident atoms stop their cell at step 0
    Cells b;
    b.add(5.64, {0.25, 0.5, 0.75, 0.6, 0.1, 0.7, 1.25, 0.5, 0.75}, {0, 1, 0});
    Result out;
    CHECK(call(b, Run(), &out) == 0, "%s", egnn_last_error());
    CHECK(out.status[0] == 3 && out.steps[0] == 0, "coincident: status %d", out.status[0]);
  }
  {   // the step alone: cells of 1, 257 and 0 atoms
    const int32_t cell_ptr[4] = {0, 1, 258, 258};
    const int N = 258, C = 3, max_steps = 3;
    std::vector<double> lattice, force(3 * N), frac(3 * N), v(3 * N, 0.0), since(3 * N, 0.0), moved(3 * N, 0.0), scalars(5 * C, 0.0),
        energy(C, -1.0), e_trace((max_steps + 1) * C, NAN), f_trace((max_steps + 1) * C, NAN);
    for (int c = 0; c < C; ++c) lattice.insert(lattice.end(), kThin, kThin + 9);
    for (int t = 0; t < 3 * N; ++t) { force[t] = 2.0 * uniform() - 1.0; frac[t] = uniform(); }
    for (int c = 0; c < C; ++c) { scalars[5 * c] = 0.1; scalars[5 * c + 1] = 0.1; }
    std::vector<int32_t> counters(4 * C, 0), done(C, 0), rebuild(C, 0), coincident(C, 0);
    for (int k = 0; k < 6; ++k) {
      CHECK(egnn_cell_relax_step_host(C, N, cell_ptr, lattice.data(), force.data(), energy.data(), coincident.data(), 1.0, 5, 1.1, 0.5, 0.1, 0.99,
                                      0.2, 1e-3, max_steps, 0.5, frac.data(), v.data(), since.data(), moved.data(), scalars.data(),
                                      counters.data(), done.data(), rebuild.data(), e_trace.data(), f_trace.data()) == 0, "%s", egnn_last_error());
      for (int c = 0; c < C; ++c)
        if (rebuild[c]) {
          rebuild[c] = 0;
          for (int t = 3 * cell_ptr[c]; t < 3 * cell_ptr[c + 1]; ++t) since[t] = 0.0;
        }
    }
    CHECK(done[0] && done[1] && done[2] && counters[4 * 0 + 2] == 2 && counters[4 * 1 + 1] == max_steps && counters[4 * 2 + 2] == 1, "the step alone");
    CHECK(egnn_cell_relax_step_host(C, N + 1, cell_ptr, lattice.data(), force.data(), energy.data(), coincident.data(), 1.0, 5, 1.1, 0.5, 0.1, 0.99,
                                    0.2, 1e-3, max_steps, 0.5, frac.data(), v.data(), since.data(), moved.data(), scalars.data(), counters.data(),
                                    done.data(), rebuild.data(), nullptr, nullptr) == EGNN_EINVAL, "cell_ptr that does not end at N");
  }
  {   // bad arguments
    Result out;
    auto bad = [&](const char* what, void (*change)(Run&)) {
      Run r;
      r.max_steps = 2;
      change(r);
      CHECK(call(salt, r, &out) == EGNN_EINVAL, "%s", what);
    };
    bad("f_max = 0", [](Run& r) { r.f_max = 0.0; });
    bad("f_max = NaN", [](Run& r) { r.f_max = NAN; });
    bad("max_steps = -1", [](Run& r) { r.max_steps = -1; });
    bad("skin = 0", [](Run& r) { r.skin = 0.0; });
    bad("max_step above skin / 2", [](Run& r) { r.max_step = 0.21; });
    bad("max_step = 0", [](Run& r) { r.max_step = 0.0; });
    bad("f_dec = 1", [](Run& r) { r.f_dec = 1.0; });
    bad("short_cut above r_cut", [](Run& r) { r.short_cut = 6.1; });
    bad("a width below (r_cut + skin) / 4", [](Run& r) { r.skin = 16.6; r.max_step = 0.2; });
  }
  printf("CELL-RELAX-OK\n");
  return 0;
}
