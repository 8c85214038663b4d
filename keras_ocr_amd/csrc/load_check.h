// load_check.h — what kocr_load_craft / kocr_load_crnn ask of a weight set, checked on the host before the context is touched.
// Host only: nothing of HIP is included, so that scripts/host_load_check.cpp can call the two functions as they are.
//
// Both take the set as name -> element count and return the empty string for a complete set, else the refusal's text naming
// the first offending tensor ("missing tensor <name>" / "tensor <name> has wrong size").  A load is refused as a whole: the
// loaders change nothing of the context until the set has passed (include/kocr.h at kocr_load_craft).
#pragma once
#include <cstddef>
#include <map>
#include <string>

using BlobSizes = std::map<std::string, size_t>;

// one convolution of the detector (detection.py:65-103, 312-335, 353-413): its Keras layer name, its BatchNorm's (or nullptr)
struct CraftSpec {
  const char* conv;
  const char* bn;  // nullptr: no BN
  int cin, cout, k, dil, relu;
};

inline constexpr CraftSpec kCraftSpecs[] = {
    {"basenet.slice1.0", "basenet.slice1.1", 3, 64, 3, 1, 1},
    {"basenet.slice1.3", "basenet.slice1.4", 64, 64, 3, 1, 1},
    {"basenet.slice1.7", "basenet.slice1.8", 64, 128, 3, 1, 1},
    {"basenet.slice1.10", "basenet.slice1.11", 128, 128, 3, 1, 1},
    {"basenet.slice2.14", "basenet.slice2.15", 128, 256, 3, 1, 1},
    {"basenet.slice2.17", "basenet.slice2.18", 256, 256, 3, 1, 1},
    {"basenet.slice3.20", "basenet.slice3.21", 256, 256, 3, 1, 1},
    {"basenet.slice3.24", "basenet.slice3.25", 256, 512, 3, 1, 1},
    {"basenet.slice3.27", "basenet.slice3.28", 512, 512, 3, 1, 1},
    {"basenet.slice4.30", "basenet.slice4.31", 512, 512, 3, 1, 1},
    {"basenet.slice4.34", "basenet.slice4.35", 512, 512, 3, 1, 1},
    // s4 is the BN output, NOT its ReLU (detection.py:333)
    {"basenet.slice4.37", "basenet.slice4.38", 512, 512, 3, 1, 0},
    {"basenet.slice5.1", nullptr, 512, 1024, 3, 6, 0},
    {"basenet.slice5.2", nullptr, 1024, 1024, 1, 1, 0},
    {"upconv1.conv.0", "upconv1.conv.1", 1536, 512, 1, 1, 1},
    {"upconv1.conv.3", "upconv1.conv.4", 512, 256, 3, 1, 1},
    {"upconv2.conv.0", "upconv2.conv.1", 768, 256, 1, 1, 1},
    {"upconv2.conv.3", "upconv2.conv.4", 256, 128, 3, 1, 1},
    {"upconv3.conv.0", "upconv3.conv.1", 384, 128, 1, 1, 1},
    {"upconv3.conv.3", "upconv3.conv.4", 128, 64, 3, 1, 1},
    {"upconv4.conv.0", "upconv4.conv.1", 192, 64, 1, 1, 1},
    {"upconv4.conv.3", "upconv4.conv.4", 64, 32, 3, 1, 1},
    {"conv_cls.0", nullptr, 32, 32, 3, 1, 1},
    {"conv_cls.2", nullptr, 32, 32, 3, 1, 1},
    {"conv_cls.4", nullptr, 32, 16, 3, 1, 1},
    {"conv_cls.6", nullptr, 16, 16, 1, 1, 1},
    {"conv_cls.8", nullptr, 16, 2, 1, 1, 0},
};

namespace load_check {
// "" when `name` is there with `numel` elements (0: any size), else the refusal
inline std::string need(const BlobSizes& blobs, const std::string& name, size_t numel) {
  auto it = blobs.find(name);
  if (it == blobs.end()) return "missing tensor " + name;
  if (numel && it->second != numel) return "tensor " + name + " has wrong size";
  return "";
}
}  // namespace load_check

// The detector's set (names without a "module." prefix), in the order craft_load reads it.
inline std::string craft_check_blobs(const BlobSizes& blobs) {
  std::string bad;
  for (const CraftSpec& s : kCraftSpecs) {
    const std::string conv = s.conv;
    if (!(bad = load_check::need(blobs, conv + ".weight", (size_t)s.cout * s.cin * s.k * s.k)).empty()) return bad;
    if (!(bad = load_check::need(blobs, conv + ".bias", (size_t)s.cout)).empty()) return bad;
    if (s.bn)
      for (const char* part : {".weight", ".bias", ".running_mean", ".running_var"})
        if (!(bad = load_check::need(blobs, std::string(s.bn) + part, (size_t)s.cout)).empty()) return bad;
  }
  return "";
}

// The recogniser's set (default build parameters, recognition.py:13-23), in the order crnn_load reads it.  *n_classes: the
// length of fc_12/bias.  *stn: whether the set carries the localisation network -- all eight stn_* tensors or none of them
// (build_params["stn"] = False, recognition.py:243); a set with some of them is refused naming the first that is missing.
inline std::string crnn_check_blobs(const BlobSizes& blobs, int* n_classes, bool* stn) {
  constexpr size_t UNITS = 128;
  const size_t filters[7] = {64, 128, 256, 256, 512, 512, 512};
  std::string bad;
  size_t cin = 1;
  for (int i = 1; i <= 7; ++i) {
    const size_t cout = filters[i - 1];
    const std::string nm = "conv_" + std::to_string(i);
    if (!(bad = load_check::need(blobs, nm + "/kernel", 9 * cin * cout)).empty()) return bad;
    if (!(bad = load_check::need(blobs, nm + "/bias", cout)).empty()) return bad;
    if (i == 3 || i == 5 || i == 7)
      for (const char* part : {"/gamma", "/beta", "/moving_mean", "/moving_variance"})
        if (!(bad = load_check::need(blobs, "bn_" + std::to_string(i) + part, cout)).empty()) return bad;
    cin = cout;
  }
  const struct {
    const char* name;
    size_t numel;
  } stn_set[8] = {{"stn_conv_1/kernel", (size_t)25 * 512 * 16}, {"stn_conv_1/bias", 16},  {"stn_conv_2/kernel", (size_t)25 * 16 * 32},
                  {"stn_conv_2/bias", 32},                      {"stn_dense_1/kernel", (size_t)11200 * 64}, {"stn_dense_1/bias", 64},
                  {"stn_dense_2/kernel", (size_t)64 * 6},       {"stn_dense_2/bias", 6}};
  bool any = false;
  for (const auto& kv : blobs) any = any || kv.first.rfind("stn_", 0) == 0;
  if (any)
    for (const auto& t : stn_set)
      if (!(bad = load_check::need(blobs, t.name, t.numel)).empty()) return bad;
  if (!(bad = load_check::need(blobs, "fc_9/kernel", 3584 * UNITS)).empty()) return bad;
  if (!(bad = load_check::need(blobs, "fc_9/bias", UNITS)).empty()) return bad;
  for (const char* l : {"lstm_10", "lstm_10_back", "lstm_11", "lstm_11_back"}) {
    if (!(bad = load_check::need(blobs, std::string(l) + "/kernel", UNITS * 4 * UNITS)).empty()) return bad;
    if (!(bad = load_check::need(blobs, std::string(l) + "/bias", 4 * UNITS)).empty()) return bad;
    if (!(bad = load_check::need(blobs, std::string(l) + "/recurrent_kernel", UNITS * 4 * UNITS)).empty()) return bad;
  }
  if (!(bad = load_check::need(blobs, "fc_12/bias", 0)).empty()) return bad;
  const size_t classes = blobs.find("fc_12/bias")->second;
  if (classes < 1) return "tensor fc_12/bias has wrong size";
  if (!(bad = load_check::need(blobs, "fc_12/kernel", 2 * UNITS * classes)).empty()) return bad;
  *n_classes = (int)classes;
  *stn = any;
  return "";
}
