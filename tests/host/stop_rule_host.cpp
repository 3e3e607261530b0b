// TEST INFRASTRUCTURE: the loop's stop rule (bayespy_amd/csrc/vmp_stop_rule.h) compiled for the
// host, so that a CPU test can set it against the Python expression of VB._end_iteration_step.
#include "vmp_stop_rule.h"

extern "C" {

int stop_rule(double L, double L0, double tol) { return vmp_stop_rule(L, L0, tol); }

double bound_sum(const double *terms, const int *order, int norder)
{
    return vmp_bound_sum(terms, order, norder);
}

}
