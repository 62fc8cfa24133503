// Same include path as the reference's src/misc/BoundaryValueProblem/BVPSchurComplementMatrices.cuh.  In this build the factors and matrices of that
// header are tables the library computes on the host (uammd_amd/csrc/bvp_host.hpp) and the solve is one device function
// (device/BVP.hip.hpp); user code reaches both through BVPSolver.cuh.
#pragma once
#include "BVPSolver.cuh"
