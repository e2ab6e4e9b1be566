// times build_row_table (host classification) for BASELINE config 2 / 3 grids -- no GPU needed
//   time_classify [reps]   best of reps (default 5) builds per grid
//   time_classify --dump   every row and layout field of the row tables of a grid of calls (mothers, precisions, lengths,
//                          tolerances, batches, options), one fresh plan each: the dumps of two commits must be equal
//                          where classification is meant to be unchanged
#include "plan.hpp"
#include <chrono>
using namespace cwtd;

namespace {
// One call of build_row_table; rows_per_signal > 0: a batch of nrows / rows_per_signal signals
struct Call {
  int mother; double param; const double *a, *amp_re, *amp_im; int64_t spec_ld; int nrows;
  const int *tab_klo = nullptr, *tab_nband = nullptr; int rows_per_signal = 0; int64_t tab_ld = -1, ols_ncols = 0, out_ncols = 0;
};
int build(cwt_plan* p, const Call& c) {
  RowRequest r;
  r.mother = c.mother; r.param = c.param; r.a = c.a; r.amp_re = c.amp_re; r.amp_im = c.amp_im; r.spec_ld = c.spec_ld;
  r.nrows = c.nrows; r.tab_klo = c.tab_klo; r.tab_nband = c.tab_nband; r.rows_per_signal = c.rows_per_signal;
  r.tab_ld = c.tab_ld; r.ols_ncols = c.ols_ncols; r.out_ncols = c.out_ncols;
  return build_row_table(p, r);
}

// a plan as cwt_plan_create leaves it (no device resources)
cwt_plan* new_plan(int logn, int prec, int max_rows = 256) {
  cwt_plan* p = new cwt_plan();
  p->N = int64_t(1) << logn; p->logN = logn; p->prec = prec; p->max_rows = max_rows; p->log_wg_points = prec == 64 ? 13 : 14;
  p->narrow_terms = prec == 64 ? 4 : 8; p->serial_rows = prec == 64 ? 2 : 0; p->narrow_mix = prec == 64; p->ols_big = prec == 32;
  return p;
}

// filter parameters of rows scales, log-spaced from the smallest resolvable scale to N (dt = 1), as prepare_table makes them
void scale_grid(const cwt_plan* p, int mother, double param, int rows, int rep, std::vector<double>& a, std::vector<double>& ar,
                std::vector<double>& ai) {
  const double pi = 3.14159265358979323846;
  const double fl = mother == 0 ? 4 * pi / (param + std::sqrt(2 + param * param)) : mother == 1 ? 4 * pi / (2 * param + 1) : 2 * pi / std::sqrt(param + 0.5);
  const double s0 = 2.0 / fl, dj = std::log2(double(p->N) / s0) / (rows - 1);
  a.resize(rows); ar.resize(rows); ai.resize(rows);
  double cre, cim; mother_constant(mother, param, &cre, &cim);
  const double w1 = 2 * pi / double(p->N);
  for (int j = 0; j < rows; ++j) { const double s = s0 * std::pow(2.0, j * dj) * (1 + rep * 1e-13); a[j] = s * w1; const double n = std::sqrt(s * w1 * p->N); ar[j] = n * cre; ai[j] = n * cim; }
}

void dump_table(const char* name, const cwt_plan* p, int rc) {
  printf("== %s rc %d\n", name, rc);
  if (rc) { printf("err %s\n", g_err.c_str()); return; }
  const auto* t = p->rt;
  for (const RowDesc& r : t->table)
    printf("row %a %a %a %d %d %d %d %d %d %ld %ld %ld %ld %a %a\n", r.a, r.amp_re, r.amp_im, r.k_lo, r.nband, r.out_row, r.logK,
           r.nterms, r.kc_off, r.rtab_off, r.spec_off, r.tab_off, r.aux_off, r.nyq_re, r.nyq_im);
  printf("counts small %d narrow %d wide %d wide_first %d ols %d ols_first %d aols %d aols_first %d aux_first %d aols2 %d aols2_first %d poly %d poly_first %d\n",
         t->n_small, t->n_narrow, t->n_wide, t->wide_first, t->n_ols, t->ols_first, t->n_aols, t->aols_first, t->aux_first, t->n_aols2,
         t->aols2_first, t->n_poly, t->poly_first);
  for (const auto& g : t->narrow_groups) printf("narrow_group %d %d %d %d\n", g.logK, g.first, g.count, g.nterms);
  for (int g = 0; g < 2; ++g) {
    const auto& G = t->ols_grp[g];
    printf("ols_grp %d logp %d n %d wgs %ld wgs_base %ld fwd %ld %ld rows %d %d wg_first", g, G.logp, G.cls.n, G.wgs, G.wgs_base,
           G.fwd_blocks[0], G.fwd_blocks[1], G.row_first, G.nrows);
    for (int i = 0; i < OLS_MAX_CLASSES; ++i) printf(" %d", G.cls.wg_first[i]);
    printf("\n");
    for (int i = 0; i < G.cls.n; ++i) {
      const OlsClass& k = G.cls.c[i];
      printf("  ols_class %d %d %d %d %d %d %d %d %ld\n", k.wg_first, k.blk_first, k.nblocks, k.nrows, k.row_first, k.halo, k.logb,
             k.nsig, k.xs_off);
    }
  }
  printf("ols elems xs %ld gt %ld nbatch %d xs_sig %ld\n", t->ols_xs_elems, t->ols_gt_elems, t->ols_nbatch, t->ols_xs_sig);
  const AolsGeom* gs[2] = {&t->aols_geom, &t->aols2_geom};
  for (const AolsGeom* g : gs)
    printf("aols_geom %d %d %d %d %a %a %a %a %a\n", g->nrows, g->nblocks, g->halo, g->ksp, g->f_s, g->f1_lo, g->z, g->zc_c, g->zc_w);
  printf("aols logp %d nbatch %d wgs %ld wgs2 %ld gt %ld\n", t->aols_logp, t->aols_nbatch, t->aols_wgs, t->aols2_wgs, t->aols_gt_elems);
  for (const auto& ch : t->poly_chunks) {
    printf("poly_chunk %d %d %d wgs %ld %ld %ld\n", ch.row_first, ch.nrows, ch.max_logk, ch.wgs[0], ch.wgs[1], ch.wgs[2]);
    for (int i = 0; i < ch.cls.n; ++i) {
      const PolyClass& c = ch.cls.c[i];
      printf("  poly_class %d %d %d %d %d\n", c.logK, c.row_first, c.nrows, c.ndeg, c.wg_first);
    }
  }
  for (const auto& r : t->poly_rtabs) printf("poly_rtab %d %d %ld\n", r.logK, r.deg, r.off);
  printf("poly elems coef %ld band %ld rtab %ld\n", t->poly_coef_elems, t->poly_band_elems, t->poly_rtab_elems);
}

int dump() {
  struct Mo { int mother; double param; const char* name; } mothers[] = {
    {0, 6.0, "morlet6"}, {1, 4.0, "paul4"}, {2, 2.0, "dog2"}, {2, 1.0, "dog1"}, {2, 0.0, "dog0"}};
  struct Opt { const char* name; void (*set)(cwt_plan*); } opts[] = {
    {"base", [](cwt_plan*) {}},
    {"poly=0", [](cwt_plan* p) { p->poly = 0; }}, {"ols=0", [](cwt_plan* p) { p->ols = 0; }},
    {"aols_zc=0", [](cwt_plan* p) { p->aols_zc = 0; }}, {"aols_long=0", [](cwt_plan* p) { p->aols_long = 0; }},
    {"ols_small_max_halo=0", [](cwt_plan* p) { p->ols_small_max_halo = 0; }},
    {"poly_cheb=0", [](cwt_plan* p) { p->poly_cheb = 0; }}, {"poly_chunk_mb=0", [](cwt_plan* p) { p->poly_chunk_mb = 0; }},
    {"narrow_mix^", [](cwt_plan* p) { p->narrow_mix = !p->narrow_mix; }}};
  char name[256];
  std::vector<double> a, ar, ai;
  for (const Opt& o : opts)
    for (int prec : {64, 32})
      for (const Mo& m : mothers)
        for (int logn : {12, 16, 18, 20, 23}) {
          if (&o != &opts[0] && (logn == 12 || logn == 18)) continue;   // option variants: 2^16, 2^20, 2^23
          for (double tol : {0.0, 1e-9})
            for (int sig : {1, 0}) {
              if (&o != &opts[0] && !sig) continue;
              cwt_plan* p = new_plan(logn, prec);
              p->tolerance = tol;
              o.set(p);
              scale_grid(p, m.mother, m.param, 96, 0, a, ar, ai);
              Call c{m.mother, m.param, a.data(), ar.data(), ai.data(), 0, 96};
              c.ols_ncols = sig ? p->N : 0;
              c.out_ncols = p->N;
              snprintf(name, sizeof name, "%s %s fp%d 2^%d tol %g signal %d", o.name, m.name, prec, logn, tol, sig);
              dump_table(name, p, build(p, c));
              delete p;
            }
        }
  // batches of 4 signals: cwt_transform_batch (signals at hand) and cwt_transform_rows_batch (spectra only)
  for (int prec : {64, 32})
    for (const Mo& m : mothers)
      for (int logn : {16, 18})
        for (double tol : {0.0, 1e-9})
          for (int sig : {1, 0}) {
            cwt_plan* p = new_plan(logn, prec);
            p->tolerance = tol;
            scale_grid(p, m.mother, m.param, 48, 0, a, ar, ai);
            std::vector<double> ba, br, bi;
            for (int b = 0; b < 4; ++b) { ba.insert(ba.end(), a.begin(), a.end()); br.insert(br.end(), ar.begin(), ar.end()); bi.insert(bi.end(), ai.begin(), ai.end()); }
            Call c{m.mother, m.param, ba.data(), br.data(), bi.data(), p->N, 4 * 48};
            c.rows_per_signal = 48;
            c.ols_ncols = c.out_ncols = sig ? p->N : 0;
            snprintf(name, sizeof name, "batch4 %s fp%d 2^%d tol %g signal %d", m.name, prec, logn, tol, sig);
            dump_table(name, p, build(p, c));
            delete p;
          }
  // a filter bank of the caller's, shaped like bluestein_convolve's
  for (int prec : {64, 32})
    for (int logn : {12, 20}) {
      cwt_plan* p = new_plan(logn, prec);
      const int nrows = 8;
      std::vector<double> one(nrows, 1.0), zero(nrows, 0.0);
      std::vector<int> klo(nrows, int(-(p->N / 2))), nb(nrows, int(p->N));
      Call c{MOTHER_TABLE, 0.0, one.data(), one.data(), zero.data(), p->N, nrows};
      c.tab_klo = klo.data(); c.tab_nband = nb.data(); c.tab_ld = 0;
      snprintf(name, sizeof name, "table fp%d 2^%d", prec, logn);
      dump_table(name, p, build(p, c));
      delete p;
    }
  // the BASELINE grids of the timing mode
  for (int logn : {20, 23})
    for (const Mo& m : mothers) {
      cwt_plan* p = new_plan(logn, 64);
      p->tolerance = 3.16e-10;
      scale_grid(p, m.mother, m.param, 77, 0, a, ar, ai);
      Call c{m.mother, m.param, a.data(), ar.data(), ai.data(), p->N, 77};   // per-row spectra (the smoothing rows)
      snprintf(name, sizeof name, "rowspectra %s 2^%d", m.name, logn);
      dump_table(name, p, build(p, c));
      delete p;
    }
  // errors
  {
    cwt_plan* p = new_plan(16, 64);
    scale_grid(p, 0, 6.0, 8, 0, a, ar, ai);
    a[3] = -1.0;
    Call c{0, 6.0, a.data(), ar.data(), ai.data(), 0, 8};
    dump_table("error scale", p, build(p, c));
    c.mother = 7;
    dump_table("error mother", p, build(p, c));
    delete p;
  }
  // one slot rebuilt: polynomial rows (fp64 Paul at 2^20), then a call without (DOG(0) rows of a batch of 4 spectra)
  {
    cwt_plan* p = new_plan(20, 64);
    p->tolerance = 1e-9;
    scale_grid(p, 1, 4.0, 96, 0, a, ar, ai);
    Call c{1, 4.0, a.data(), ar.data(), ai.data(), 0, 96};
    c.ols_ncols = c.out_ncols = p->N;
    dump_table("rebuild 1: paul4 fp64 2^20", p, build(p, c));
    scale_grid(p, 2, 0.0, 24, 0, a, ar, ai);
    std::vector<double> ba, br, bi;
    for (int b = 0; b < 4; ++b) { ba.insert(ba.end(), a.begin(), a.end()); br.insert(br.end(), ar.begin(), ar.end()); bi.insert(bi.end(), ai.begin(), ai.end()); }
    Call d{2, 0.0, ba.data(), br.data(), bi.data(), p->N, 4 * 24};
    d.rows_per_signal = 24;
    dump_table("rebuild 2: dog0 fp64 2^20 batch of 4 spectra, same slot", p, build(p, d));
    delete p;
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--dump") return dump();
  struct Cfg { const char* name; int mother; double param; int prec; double tol; int logn = 20; int rows = 256; long spec_ld = 0; } cfgs[] = {
    {"c2", 0, 6.0, 64, 1e-9}, {"c3_paul", 1, 4.0, 32, 3e-5}, {"c3_dog", 2, 2.0, 32, 3e-5}, {"paul64", 1, 4.0, 64, 1e-9}, {"c2_roundoff", 0, 6.0, 64, 1e-16},
    {"mc_2^23_77", 0, 6.0, 64, 3.16e-10, 23, 77}, {"mc_2^23_77b", 0, 6.0, 64, 1e-9, 23, 77},
    {"smooth_2^23", 2, 0.0, 64, 3.16e-10, 23, 77, 1L << 23}, {"smooth_2^23b", 2, 0.0, 64, 1e-9, 23, 77, 1L << 23}};
  for (auto& c : cfgs) {
    cwt_plan* p = new cwt_plan();
    p->N = 1 << c.logn; p->logN = c.logn; p->prec = c.prec; p->max_rows = 256; p->log_wg_points = c.prec == 64 ? 13 : 14;
    p->narrow_terms = c.prec == 64 ? 4 : 8; p->narrow_mix = c.prec == 64; p->ols_big = c.prec == 32; p->tolerance = c.tol;
    const int rows = c.rows;
    std::vector<double> a, ar, ai;
    double best = 1e9;
    for (int rep = 0; rep < (argc > 1 ? atoi(argv[1]) : 5); ++rep) {
      scale_grid(p, c.mother, c.param, rows, rep, a, ar, ai);
      p->rt = &p->slots[rep & 1];
      Call call{c.mother, c.param, a.data(), ar.data(), ai.data(), c.spec_ld, rows};
      call.ols_ncols = call.out_ncols = p->N;
      auto t0 = std::chrono::steady_clock::now();
      int rc = build(p, call);
      double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (rc) { printf("rc %d %s\n", rc, g_err.c_str()); return 1; }
      best = std::min(best, ms);
      if (rep == 0) printf("   first call %.1f ms\n", ms);
    }
    set_split(p);
    printf("%-12s build_row_table %.3f ms  (poly %d ols %d aols %d wide %d) planes %.1f MB in %zu chunks, bands %.1f MB\n", c.name, best, p->rt->n_poly, p->rt->n_ols, p->rt->n_aols, p->rt->n_wide, p->rt->poly_coef_elems * (c.prec == 64 ? 16.0 : 8.0) / 1e6, p->rt->poly_chunks.size(), p->rt->poly_band_elems * (c.prec == 64 ? 16.0 : 8.0) / 1e6);
  }
  return 0;
}
