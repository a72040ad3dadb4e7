// Greedy C/F splitting by diagonal dominance (ns/lib/greedy.py:13-36), host only: plain C++ on
// host CSR arrays, no device call. greedy.cpp is part of libmlamg_hip.so and is also compiled on
// its own with tests/host/greedy_driver.cpp (tests/test_greedy_host.py), which supplies
// set_error.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mlamg.h"

namespace mlamg {

void set_error(const std::string& msg);

// The splitting itself, arguments already validated: F and C in the reference's append order.
void greedy_split(int64_t n, const int32_t* indptr, const int32_t* indices, const double* data,
                  double theta, std::vector<int32_t>& F, std::vector<int32_t>& C);

}  // namespace mlamg
