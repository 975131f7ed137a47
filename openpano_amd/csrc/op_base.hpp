// op_base.hpp -- what every translation unit of libopenpano_hip.so sees, with or without the HIP runtime: the error path
#pragma once
#include <string>
#include "openpano_hip.h"

#define OP_MAX_KCENTER 15    // Gaussian kernels up to 31 taps

void op_set_error(const std::string& msg);
#define OP_FAIL(code, msg) do { op_set_error(msg); return (code); } while (0)
