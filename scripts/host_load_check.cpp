// Developer check on the host alone (no GPU, nothing of the library linked): (1) the two validation functions that
// kocr_load_craft / kocr_load_crnn run before they touch a context (load_check.h) on complete weight sets and on sets with each
// defect that tests/lifecycle_cases.py offers a live context; (2) the sized list of a context's persistent allocations
// (common.h: dev_alloc, release, release_since -- what TempLayer's destructor calls behind its stream synchronisation) with
// malloc / free standing in for the counted allocator of api.cpp.  Under the address and undefined-behaviour sanitizers a
// double free, a leak or a use after release is reported.
//   hipcc -std=c++17 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Wno-unused-value -I keras_ocr_amd/csrc \
//         scripts/host_load_check.cpp -o host_load_check && ./host_load_check
#include "common.h"
#include "load_check.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
      exit(1);                                        \
    }                                                 \
  } while (0)

// ---- the counted allocator of api.cpp, restated on host memory ----
static size_t g_count = 0, g_bytes = 0;
static std::map<void*, size_t> g_size;
hipError_t kocr_counted_malloc(void** p, size_t bytes) {
  *p = malloc(bytes);
  g_size[*p] = bytes;
  ++g_count;
  g_bytes += bytes;
  return hipSuccess;
}
hipError_t kocr_counted_free(void* p) {
  if (!p) return hipSuccess;
  CHECK(g_size.count(p) == 1);  // freed once, and only what was allocated here
  --g_count;
  g_bytes -= g_size[p];
  g_size.erase(p);
  free(p);
  return hipSuccess;
}

// ---- complete weight sets, by the shapes of weights.synthetic_craft_weights / synthetic_crnn_weights ----
static BlobSizes craft_set() {
  BlobSizes b;
  for (const CraftSpec& s : kCraftSpecs) {
    b[std::string(s.conv) + ".weight"] = (size_t)s.cout * s.cin * s.k * s.k;
    b[std::string(s.conv) + ".bias"] = (size_t)s.cout;
    if (s.bn)
      for (const char* part : {".weight", ".bias", ".running_mean", ".running_var"}) b[std::string(s.bn) + part] = (size_t)s.cout;
  }
  return b;
}

static BlobSizes crnn_set(size_t classes, bool stn) {
  BlobSizes b;
  const size_t f[7] = {64, 128, 256, 256, 512, 512, 512};
  size_t cin = 1;
  for (int i = 1; i <= 7; ++i) {
    const std::string nm = "conv_" + std::to_string(i);
    b[nm + "/kernel"] = 9 * cin * f[i - 1];
    b[nm + "/bias"] = f[i - 1];
    if (i == 3 || i == 5 || i == 7)
      for (const char* part : {"/gamma", "/beta", "/moving_mean", "/moving_variance"}) b["bn_" + std::to_string(i) + part] = f[i - 1];
    cin = f[i - 1];
  }
  if (stn) {
    b["stn_conv_1/kernel"] = 25 * 512 * 16;
    b["stn_conv_1/bias"] = 16;
    b["stn_conv_2/kernel"] = 25 * 16 * 32;
    b["stn_conv_2/bias"] = 32;
    b["stn_dense_1/kernel"] = 11200 * 64;
    b["stn_dense_1/bias"] = 64;
    b["stn_dense_2/kernel"] = 64 * 6;
    b["stn_dense_2/bias"] = 6;
  }
  b["fc_9/kernel"] = 3584 * 128;
  b["fc_9/bias"] = 128;
  for (const char* l : {"lstm_10", "lstm_10_back", "lstm_11", "lstm_11_back"}) {
    b[std::string(l) + "/kernel"] = 128 * 512;
    b[std::string(l) + "/recurrent_kernel"] = 128 * 512;
    b[std::string(l) + "/bias"] = 512;
  }
  b["fc_12/kernel"] = 256 * classes;
  b["fc_12/bias"] = classes;
  return b;
}

static BlobSizes without(BlobSizes b, const char* name) {
  CHECK(b.erase(name) == 1);
  return b;
}
static BlobSizes resized(BlobSizes b, const char* name) {
  CHECK(b.count(name) == 1);
  b[name] += 1;
  return b;
}

int main() {
  // (1a) the recogniser's sets
  int C = -1;
  bool stn = false;
  CHECK(crnn_check_blobs(crnn_set(37, true), &C, &stn).empty() && C == 37 && stn);
  CHECK(crnn_check_blobs(crnn_set(96, false), &C, &stn).empty() && C == 96 && !stn);
  CHECK(crnn_check_blobs(crnn_set(1, true), &C, &stn).empty() && C == 1);
  for (const char* name : {"conv_1/kernel", "bn_5/gamma", "lstm_11_back/recurrent_kernel", "fc_12/kernel", "fc_12/bias", "fc_9/bias",
                           "lstm_10/kernel", "conv_7/bias", "bn_7/moving_variance"}) {
    C = -1;
    CHECK(crnn_check_blobs(without(crnn_set(37, true), name), &C, &stn) == std::string("missing tensor ") + name);
    CHECK(C == -1);  // a refusal reports nothing else
    CHECK(crnn_check_blobs(without(crnn_set(37, false), name), &C, &stn) == std::string("missing tensor ") + name);
  }
  for (const char* name : {"conv_4/kernel", "conv_1/kernel", "bn_3/beta", "fc_9/kernel", "lstm_10_back/bias", "stn_dense_1/kernel"})
    CHECK(crnn_check_blobs(resized(crnn_set(37, true), name), &C, &stn) == std::string("tensor ") + name + " has wrong size");
  // fc_12: the kernel must fit the class count that the bias states
  CHECK(crnn_check_blobs(resized(crnn_set(37, true), "fc_12/kernel"), &C, &stn) == "tensor fc_12/kernel has wrong size");
  CHECK(crnn_check_blobs(resized(crnn_set(37, true), "fc_12/bias"), &C, &stn) == "tensor fc_12/kernel has wrong size");
  // the stn_* tensors: all eight or none
  for (const char* name : {"stn_dense_2/bias", "stn_conv_1/kernel", "stn_conv_2/bias", "stn_dense_1/kernel"})
    CHECK(crnn_check_blobs(without(crnn_set(37, true), name), &C, &stn) == std::string("missing tensor ") + name);
  {
    BlobSizes one = crnn_set(37, false);
    one["stn_dense_2/bias"] = 6;
    CHECK(crnn_check_blobs(one, &C, &stn) == "missing tensor stn_conv_1/kernel");
  }
  {
    BlobSizes extra = crnn_set(37, true);  // tensors the loader does not know are ignored
    extra["dropout/rate"] = 1;
    CHECK(crnn_check_blobs(extra, &C, &stn).empty());
  }
  CHECK(crnn_check_blobs(BlobSizes{}, &C, &stn) == "missing tensor conv_1/kernel");

  // (1b) the detector's sets
  CHECK(craft_check_blobs(craft_set()).empty());
  for (const char* name : {"basenet.slice1.0.weight", "upconv1.conv.1.running_var", "conv_cls.8.bias", "basenet.slice5.2.weight",
                           "basenet.slice4.38.running_mean", "upconv4.conv.4.bias"})
    CHECK(craft_check_blobs(without(craft_set(), name)) == std::string("missing tensor ") + name);
  for (const char* name : {"basenet.slice3.24.weight", "conv_cls.8.weight", "upconv1.conv.0.weight", "basenet.slice1.1.weight"})
    CHECK(craft_check_blobs(resized(craft_set(), name)) == std::string("tensor ") + name + " has wrong size");
  CHECK(craft_check_blobs(BlobSizes{}) == "missing tensor basenet.slice1.0.weight");

  // (2) the sized list of persistent allocations
  {
    static kocr_ctx ctx;
    void *a = nullptr, *b = nullptr, *c = nullptr, *z = nullptr;
    CHECK(ctx.dev_alloc(&a, 100) == KOCR_OK && ctx.dev_alloc(&b, 300) == KOCR_OK && ctx.dev_alloc(&c, 7) == KOCR_OK);
    CHECK(ctx.dev_alloc(&z, 0) == KOCR_OK && z);  // an empty buffer is a real one of 4 bytes
    memset(a, 1, 100);
    memset(b, 2, 300);
    memset(c, 3, 7);
    memset(z, 4, 4);
    CHECK(ctx.owned.size() == 4 && g_count == 4 && g_bytes == 411);
    CHECK(ctx.owned[1].p == b && ctx.owned[1].bytes == 300 && ctx.owned[3].bytes == 4);
    // a middle element released: the others keep their order and their sizes
    ctx.release(b);
    CHECK(ctx.owned.size() == 3 && g_count == 3 && g_bytes == 111);
    CHECK(ctx.owned[0].p == a && ctx.owned[1].p == c && ctx.owned[1].bytes == 7 && ctx.owned[2].p == z);
    ctx.release(nullptr);  // ignored
    int not_ours = 0;
    ctx.release(&not_ours);  // a pointer the context does not own is left alone
    CHECK(ctx.owned.size() == 3 && g_count == 3);
    // the temporary layer of a kocr_conv2d_* call: what comes behind the mark goes, what was there before stays -- and so does
    // a buffer allocated before the mark that is released and replaced inside the call's lifetime
    void* early = nullptr;
    CHECK(ctx.dev_alloc(&early, 64) == KOCR_OK);  // the max-|x| slot pool's place: ahead of the mark
    const size_t mark = ctx.owned.size();
    void *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;
    CHECK(ctx.dev_alloc(&t0, 1000) == KOCR_OK && ctx.dev_alloc(&t1, 2000) == KOCR_OK && ctx.dev_alloc(&t2, 3000) == KOCR_OK);
    ctx.release(t1);  // prepare_conv releasing a copy it replaces
    CHECK(ctx.owned.size() == mark + 2 && g_bytes == 111 + 64 + 4000);
    ctx.release_since(mark);
    CHECK(ctx.owned.size() == mark && g_count == 4 && g_bytes == 175);
    CHECK(ctx.owned[0].p == a && ctx.owned[3].p == early);
    memset(early, 5, 64);  // still there
    ctx.release_since(mark);  // nothing behind the mark: nothing happens
    CHECK(ctx.owned.size() == mark);
    // the context's end
    ctx.release_since(0);
    CHECK(ctx.owned.empty() && g_count == 0 && g_bytes == 0 && g_size.empty());
  }
  printf("host_load_check ok\n");
  return 0;
}
