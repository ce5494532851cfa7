// khg_py_ebw.hpp -- what the pybind units share for the Extended Baum-Welch update: khg_ebw_results as the dict that
// DeviceModel.ebw_update (khg_pybind.cpp) and update_ebw_* / flat_ebw_update (khg_py_host.cpp) both return.
#pragma once
#include <pybind11/pybind11.h>

#include "../../include/khg_hip.h"

inline pybind11::dict EbwResultsDict(const khg_ebw_results& r) {
  pybind11::dict d;
  d["auxf_impr_gauss"] = r.auxf_impr_gauss; d["count"] = r.count; d["auxf_impr_weights"] = r.auxf_impr_weights;
  d["floored"] = r.floored; d["failed"] = r.failed; d["skipped"] = r.skipped; d["weights_skipped"] = r.weights_skipped;
  return d;
}
