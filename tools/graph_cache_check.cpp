// graph_cache_check.cpp -- PyzGraphCache (csrc/pyz_common.h) on the host alone: slot choice, eviction order, rekey, a capture
// that fails half-way, the wait before a graph launched by the same call is destroyed.  The eight HIP calls the cache makes
// are defined here (they count and hand out fake handles), so no device is needed; build for the host with the sanitizers:
//   hipcc -std=c++17 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/graph_cache_check.cpp -o graph_cache_check && ./graph_cache_check
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../bayesian_inference_for_nn_amd/csrc/pyz_common.h"

static std::set<void *> live_graphs, live_execs;
static int capturing = 0, begun = 0, syncs = 0, launches = 0, fail_end = 0;

static void *handle() { return std::malloc(1); }   // (the address sanitizer reports a handle that is never destroyed)

hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) {
  if (capturing) return hipErrorIllegalState;
  capturing = 1;
  ++begun;
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *g) {
  if (!capturing) return hipErrorIllegalState;
  capturing = 0;
  if (fail_end) return hipErrorStreamCaptureInvalidated;
  *g = (hipGraph_t)handle();
  live_graphs.insert(*g);
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *e, hipGraph_t g, hipGraphNode_t *, char *, size_t) {
  if (!live_graphs.count(g)) return hipErrorInvalidValue;
  *e = (hipGraphExec_t)handle();
  live_execs.insert(*e);
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t e, hipStream_t) {
  if (capturing || !live_execs.count(e)) return hipErrorInvalidValue;
  ++launches;
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t e) {
  if (!live_execs.erase(e)) return hipErrorInvalidValue;
  std::free(e);
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) {
  if (!live_graphs.erase(g)) return hipErrorInvalidValue;
  std::free(g);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  ++syncs;
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "stub"; }

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      return 1;                                                          \
    }                                                                    \
  } while (0)

int main() {
  const hipStream_t st = (hipStream_t)8;
  int enq = 0;
  auto steps = [&] { return capturing ? (++enq, PYZ_OK) : PYZ_E_INVALID; };   // steps are enqueued inside a capture only
  // what sgld_run_impl / pyz_hmc_run ask for: the full chunk in slot 0, remainders by exact length in slots 1 ..
  auto run = [&](PyzGraphCache<8> &c, int n) { return c.launch(n, 0, n < 32 ? 1 : 0, n < 32 ? 8 : 1, st, steps); };
  {
    PyzGraphCache<8> c;
    c.rekey(11);
    c.begin_call();
    CHECK(run(c, 32) == PYZ_OK && c.len[0] == 32 && c.captures == 1);
    for (int n = 1; n <= 7; ++n) CHECK(run(c, n) == PYZ_OK && c.len[n] == n);   // free slots first, lowest first
    CHECK(c.captures == 8 && begun == 8 && enq == 8 && launches == 8 && live_execs.size() == 8);
    c.begin_call();
    CHECK(run(c, 32) == PYZ_OK && run(c, 5) == PYZ_OK && run(c, 1) == PYZ_OK && c.captures == 0 && begun == 8 && launches == 11);
    // full: a new length replaces the least recently used remainder, never slot 0 -- lengths 2, 3, 4, 6, 7 in that order, then 5, 1
    const int order[] = {2, 3, 4, 6, 7, 5, 1};
    for (int k = 0; k < 7; ++k) {
      c.begin_call();
      CHECK(run(c, 10 + k) == PYZ_OK && c.captures == 1 && c.len[order[k]] == 10 + k && c.len[0] == 32);
    }
    CHECK(syncs == 0 && live_execs.size() == 8 && live_graphs.size() == 8);
    c.begin_call();
    CHECK(run(c, 2) == PYZ_OK && c.captures == 1 && c.len[2] == 2);   // an evicted length is captured again, over the oldest (10)
    c.rekey(11);
    CHECK(live_execs.size() == 8);   // same key: kept
    c.rekey(12);
    CHECK(live_execs.empty() && live_graphs.empty() && c.key == 12 && c.len[0] == 0);
    // a capture whose steps fail is ended, its graph destroyed, the slot left free; so is one whose end fails
    const int begun0 = begun;
    CHECK(c.launch(4, 0, 1, 8, st, [&] { return PYZ_E_SHAPE; }) == PYZ_E_SHAPE);
    CHECK(!capturing && begun == begun0 + 1 && live_graphs.empty() && live_execs.empty() && !c.exec[1] && c.captures == 1);
    fail_end = 1;
    CHECK(c.launch(4, 0, 1, 8, st, steps) == PYZ_E_HIP && !capturing && live_graphs.empty() && !c.exec[1]);
    fail_end = 0;
    CHECK(run(c, 4) == PYZ_OK && c.len[1] == 4);
    c.drop();
    CHECK(live_execs.empty() && live_graphs.empty());
  }
  {
    // signatures tell graphs of one length apart (the ADAM / BSAM runs), and a graph this call launched is waited for
    // before it is destroyed
    PyzGraphCache<2> c;
    c.rekey(1);
    c.begin_call();
    CHECK(c.launch(3, 20, 0, 2, st, steps) == PYZ_OK && c.launch(3, 21, 0, 2, st, steps) == PYZ_OK && c.captures == 2);
    CHECK(c.sig[0] == 20 && c.sig[1] == 21 && syncs == 0);
    c.begin_call();
    CHECK(c.launch(3, 21, 0, 2, st, steps) == PYZ_OK && c.captures == 0);
    CHECK(c.launch(3, 22, 0, 2, st, steps) == PYZ_OK && c.sig[0] == 22 && syncs == 0);   // slot 0: last used by an earlier call
    CHECK(c.launch(3, 23, 0, 2, st, steps) == PYZ_OK && c.sig[1] == 23 && syncs == 1);   // slot 1: launched by this call
    c.drop();
    CHECK(live_execs.empty() && live_graphs.empty());
  }
  std::puts("graph_cache_check: ok");
  return 0;
}
