// DeviceLattices of the Python surface: owns a khg_lattices handle (the raw lattices of a batch, resident on the device) and the
// context its operations run on.  Shared by khg_pybind.cpp (UtteranceSet.raw_lattices_simple_device) and khg_py_align.cpp (the class
// itself, get_raw_lattice_simple_device_batch).
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <vector>

#include "../../include/khg_hip.h"

namespace khg {

struct PyDeviceLattices {
  khg_lattices* h = nullptr;
  khg_ctx* ctx = nullptr;
  pybind11::object ctx_obj;          // keeps a Python Context alive (None: the default context)
  std::vector<int32_t> status;       // of the prune / rescore / boost / lm_rescore that made it (empty otherwise)
  bool has_rescore_stats = false;    // made by rescore: the counts of khg_rescore_stats
  khg_rescore_stats rescore_stats = {0, 0, 0};
  PyDeviceLattices() = default;
  PyDeviceLattices(const PyDeviceLattices&) = delete;
  PyDeviceLattices& operator=(const PyDeviceLattices&) = delete;
  ~PyDeviceLattices() { close(); }
  void close() { if (h) { khg_lattices_destroy(h); h = nullptr; } }
};

// DevicePosteriors: owns a khg_posteriors handle (what DeviceLattices.posteriors made, resident on the device)
struct PyDevicePosteriors {
  khg_posteriors* h = nullptr;
  khg_ctx* ctx = nullptr;
  pybind11::object ctx_obj;
  std::vector<int32_t> status;       // KHG_LAT_* bits per utterance
  std::vector<double> tot_like;
  std::vector<double> avg_acc;       // made by mpe_posteriors: the expected accuracy per utterance (empty otherwise)
  bool has_avg_acc = false;
  std::vector<int64_t> arc_off;      // of the lattices it was made from
  PyDevicePosteriors() = default;
  PyDevicePosteriors(const PyDevicePosteriors&) = delete;
  PyDevicePosteriors& operator=(const PyDevicePosteriors&) = delete;
  ~PyDevicePosteriors() { close(); }
  void close() { if (h) { khg_posteriors_destroy(h); h = nullptr; } }
};

}  // namespace khg
