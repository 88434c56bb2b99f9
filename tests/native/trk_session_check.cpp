// GPU test program for the tracker session (vpl_trk_*, include/vplines_frontend.h): the host mirror
// vplhost::LineFeatureTracker and the session run on the same frames, in one process, on two front-end contexts, with the
// same VP seed per frame.  After every call it prints, per sequence, what the mirror holds (keys m<call>_<seq>_*) and what
// the session holds and returned (keys s<call>_<seq>_*), in the key/value form of line_tracker_check.cpp, so that
// tests/test_gpu_trk_session.py can compare the two line by line.
//   usage: frames.raw n_frames W H mapx.f32 mapy.f32 max_h max_v max_lines n_seq n_calls  frame[call][seq] ...   (-1 = a blank frame)
// With VPL_DEBUG_GUARDS=1 the last line reports the guard check of both contexts.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../../vplines-slam_amd/host/vpl_frontend.hpp"

using namespace vplhost;

extern "C" int vpl_fe_debug_guards(vpl_fe_ctx*);

template <typename T>
static std::vector<T> slurp(const char* path, size_t n) {
  std::vector<T> b(n);
  FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(b.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
  std::fclose(f);
  return b;
}

static unsigned long long poly_hash(const uint8_t* p, size_t n) {
  unsigned long long sum = 0;
  for (size_t i = 0; i < n; ++i) sum = sum * 1315423911ull + p[i];
  return sum;
}

static void print_line(const float* e, const double* q, const float* c, float len) {
  std::printf(" %.9g %.9g %.9g %.9g %.17g %.17g %.17g %.9g %.9g %.9g", e[0], e[1], e[2], e[3], q[0], q[1], q[2], c[0], c[1], len);
}

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    const int rc__ = (call);                                                                          \
    if (rc__ != 0) { std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, vpl_fe_last_error(fe)); return 3; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 12) return 2;
  const int n = std::atoi(argv[2]), W = std::atoi(argv[3]), H = std::atoi(argv[4]);
  const int max_h = std::atoi(argv[7]), max_v = std::atoi(argv[8]), ML = std::atoi(argv[9]);
  const int nS = std::atoi(argv[10]), nCalls = std::atoi(argv[11]);
  if (argc < 12 + nS * nCalls) return 2;
  const size_t px = (size_t)W * H;
  std::vector<uint8_t> frames = slurp<uint8_t>(argv[1], px * n);
  std::vector<float> mx = slurp<float>(argv[5], px), my = slurp<float>(argv[6], px);
  const float fx = 458.654f, fy = 457.296f, cx = (float)(W / 2), cy = (float)(H / 2);
  const int max_kps = 16384;

  // the mirror: one device context shared by the sequences' trackers (a readImage leaves nothing on the device)
  FrontendDevice dev(W, H, ML, max_kps);
  EDLineParam param = {5, 1.0f, 30.f, 5.f, 2, 35, 1.8};
  std::vector<std::unique_ptr<LineFeatureTracker>> mir;
  uint32_t seed_now = 0;
  std::vector<int> seed_used(nS, 0);
  for (int s = 0; s < nS; ++s) {
    mir.emplace_back(new LineFeatureTracker(dev, param, max_h, max_v, true));
    mir[s]->vp_seed = [&seed_now, &seed_used, s] { seed_used[s] = 1; return seed_now; };
    mir[s]->setUndistortMaps(mx.data(), my.data(), fx, fy, cx, cy);
  }

  // the session on a context of its own
  vpl_fe_ctx* fe = nullptr;
  if (vpl_fe_create(&fe, 0, 2 * nS, W, H, ML) != 0) { std::fprintf(stderr, "vpl_fe_create failed\n"); return 3; }
  CHECK(vpl_match_reserve(fe, nS, max_kps));
  CHECK(vpl_pre_set_maps(fe, mx.data(), my.data()));
  vpl_trk_options opt;
  vpl_trk_default_options(&opt);
  opt.max_h_lines = max_h; opt.max_v_lines = max_v;
  opt.fx = fx; opt.fy = fy; opt.cx = cx; opt.cy = cy;
  vpl_trk* trk = nullptr;
  CHECK(vpl_trk_create(&trk, fe, nS, &opt));

  std::vector<uint8_t> raw(nS * px), img(px);
  std::vector<uint32_t> seeds(nS);
  std::vector<vpl_trk_result> res(nS);
  std::vector<int> ids((size_t)nS * ML), g_ids(ML), g_tc(ML), g_match(ML), g_vp(ML);
  std::vector<double> obs((size_t)nS * ML * 8);
  std::vector<vpl_line> g_lines(ML);
  std::vector<int> n_kept(nS, 0);   // lines the session's curframe_ holds (from the results)

  for (int k = 0; k < nCalls; ++k) {
    for (int s = 0; s < nS; ++s) {
      const int f = std::atoi(argv[12 + k * nS + s]);
      if (f >= n) return 2;
      if (f < 0) std::fill(raw.begin() + s * px, raw.begin() + (s + 1) * px, (uint8_t)0);
      else std::copy(frames.begin() + f * px, frames.begin() + (f + 1) * px, raw.begin() + s * px);
      seeds[s] = 1000u + 10u * k + s;
    }
    // ---- mirror ----
    for (int s = 0; s < nS; ++s) {
      LineFeatureTracker& T = *mir[s];
      seed_now = seeds[s];
      seed_used[s] = 0;
      T.readImage(raw.data() + s * px);
      const FrameLines& F = *T.curframe_;
      std::printf("m%d_%d_img", k, s);
      if (!F.vecLine.empty()) std::printf(" %llu", poly_hash(F.img.data(), px));
      std::printf("\nm%d_%d_lines", k, s);
      for (const Line& l : F.vecLine) print_line(l.line_endpoint.data(), l.line_equation.data(), l.center.data(), l.length);
      std::printf("\nm%d_%d_ids", k, s);
      for (int v : F.lineID) std::printf(" %d", v);
      std::printf("\nm%d_%d_tcnt", k, s);
      for (int v : F.t_cnt) std::printf(" %d", v);
      std::printf("\nm%d_%d_match", k, s);
      for (int v : T.last_match) std::printf(" %d", v);
      std::printf("\nm%d_%d_vpids", k, s);
      if (seed_used[s]) for (int v : T.last_vp_ids) std::printf(" %d", v);
      std::printf("\nm%d_%d_vps %d", k, s, seed_used[s]);
      for (int q = 0; q < 9; ++q) std::printf(" %.17g", seed_used[s] ? T.last_vps[q] : 0.0);
      std::printf("\nm%d_%d_obs", k, s);
      for (const auto& ob : T.lineObservations()) {
        std::printf(" %d", ob.id);
        for (int q = 0; q < 8; ++q) std::printf(" %.17g", ob.v[q]);
      }
      std::printf("\nm%d_%d_cnt %d %d %d\n", k, s, T.allfeature_cnt, T.lines_exit ? 1 : 0, (int)T.last_detected.size());
    }
    // ---- session ----
    std::vector<int> n_prev = n_kept;
    CHECK(vpl_trk_frame(trk, raw.data(), seeds.data(), res.data(), ids.data(), obs.data()));
    for (int s = 0; s < nS; ++s) {
      const vpl_trk_result& r = res[s];
      if (r.lines_exist) n_kept[s] = r.n_lines;
      int n_tc = 0;
      CHECK(vpl_trk_get_frame(trk, s, img.data(), g_lines.data(), g_ids.data(), g_tc.data(), &n_tc, g_match.data(), g_vp.data()));
      std::printf("s%d_%d_img", k, s);
      if (n_kept[s] > 0) std::printf(" %llu", poly_hash(img.data(), px));
      std::printf("\ns%d_%d_lines", k, s);
      for (int i = 0; i < n_kept[s]; ++i) print_line(g_lines[i].line_endpoint, g_lines[i].line_equation, g_lines[i].center, g_lines[i].length);
      std::printf("\ns%d_%d_ids", k, s);
      for (int i = 0; i < n_kept[s]; ++i) std::printf(" %d", g_ids[i]);
      std::printf("\ns%d_%d_tcnt", k, s);
      for (int i = 0; i < n_tc; ++i) std::printf(" %d", g_tc[i]);
      std::printf("\ns%d_%d_match", k, s);
      for (int i = 0; i < (r.matched ? n_prev[s] : 0); ++i) std::printf(" %d", g_match[i]);
      std::printf("\ns%d_%d_vpids", k, s);
      for (int i = 0; i < (r.vp_ran ? r.n_lines : 0); ++i) std::printf(" %d", g_vp[i]);
      std::printf("\ns%d_%d_vps %d", k, s, r.vp_ran);
      for (int q = 0; q < 9; ++q) std::printf(" %.17g", r.vps[q]);
      std::printf("\ns%d_%d_obs", k, s);
      for (int i = 0; i < r.n_lines; ++i) {
        std::printf(" %d", ids[(size_t)s * ML + i]);
        for (int q = 0; q < 8; ++q) std::printf(" %.17g", obs[((size_t)s * ML + i) * 8 + q]);
      }
      std::printf("\ns%d_%d_cnt %d %d %d\n", k, s, r.allfeature_cnt, r.lines_exist, r.n_detected);
      std::printf("s%d_%d_res %d %d %d %d\n", k, s, r.n_lines, r.matched, r.n_tracked, r.vp_status);
    }
  }
  const int g1 = vpl_fe_debug_guards(fe), g2 = vpl_fe_debug_guards(dev.ctx());
  std::printf("guards %d %d\n", g1, g2);
  if (g1) std::fprintf(stderr, "%s\n", vpl_fe_last_error(fe));
  vpl_trk_destroy(trk);
  vpl_fe_destroy(fe);
  return 0;
}
