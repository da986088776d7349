// mda_host.cpp: exact min-diameter subset search on the host.
#pragma once
#include <torch/extension.h>

torch::Tensor mda_search(torch::Tensor D2, int64_t f);
