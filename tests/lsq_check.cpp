// Host driver for scikit-downscale_amd/csrc/sd_lsq.h (tests/test_lsq_host.py): the text the kernels run, compiled with g++ alone.
// Numbers travel as hex floats in both directions, so nothing is rounded on the way.  One request per line on stdin:
//   minnorm F  <F rows of [S | b], row-major, F*(F+1) numbers>   ->  "coef c0 .. cF-1"
//   unresolved F n <F rows of [S | b]> <F raw sums of squares>   ->  "system <the F*(F+1) numbers after clear_unresolved>"
//   chol n     <n*n numbers of H, row-major> <n numbers of r>    ->  "ok d0 .. dn-1" or "false"
//   helpers z                                                    ->  "helpers softplus(z) sigmoid(z)"
// and "end" after the last request.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sd_lsq.h"

namespace {

bool read_numbers(std::istringstream& in, size_t count, std::vector<double>& v) {
    v.clear();
    std::string tok;
    while (v.size() < count && (in >> tok)) {
        char* end = nullptr;
        const double x = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end != '\0') return false;
        v.push_back(x);
    }
    return v.size() == count;
}

void print_numbers(const char* head, const double* v, int n) {
    std::printf("%s", head);
    for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
    std::printf("\n");
}

}  // namespace

int main() {
    std::string line;
    std::vector<double> v;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int n = 0;
        if (!(in >> what)) continue;
        if (what == "minnorm") {
            if (!(in >> n) || n < 1 || n > sdlsq::kMaxF || !read_numbers(in, (size_t)n * (n + 1), v)) return 2;
            double A[sdlsq::kMaxF][sdlsq::kMaxF + 1], coef[sdlsq::kMaxF];
            for (int f = 0; f < n; ++f)
                for (int g = 0; g <= n; ++g) A[f][g] = v[(size_t)f * (n + 1) + g];
            sdlsq::minnorm_solve(n, A, coef);
            print_numbers("coef", coef, n);
        } else if (what == "unresolved") {
            double count = 0.0;
            if (!(in >> n >> count) || n < 1 || n > sdlsq::kMaxF || !read_numbers(in, (size_t)n * (n + 2), v)) return 2;
            double A[sdlsq::kMaxF][sdlsq::kMaxF + 1], flat[sdlsq::kMaxF * (sdlsq::kMaxF + 1)];
            for (int f = 0; f < n; ++f)
                for (int g = 0; g <= n; ++g) A[f][g] = v[(size_t)f * (n + 1) + g];
            sdlsq::clear_unresolved(n, A, v.data() + (size_t)n * (n + 1), count);
            for (int f = 0; f < n; ++f)
                for (int g = 0; g <= n; ++g) flat[f * (n + 1) + g] = A[f][g];
            print_numbers("system", flat, n * (n + 1));
        } else if (what == "chol") {
            if (!(in >> n) || n < 1 || n > sdlsq::kMaxF + 1 || !read_numbers(in, (size_t)n * n + n, v)) return 2;
            double H[sdlsq::kMaxF + 1][sdlsq::kMaxF + 1], r[sdlsq::kMaxF + 1], d[sdlsq::kMaxF + 1];
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < n; ++j) H[i][j] = v[(size_t)i * n + j];
                r[i] = v[(size_t)n * n + i];
            }
            if (sdlsq::chol_solve(n, H, r, d)) print_numbers("ok", d, n);
            else std::printf("false\n");
        } else if (what == "helpers") {
            if (!read_numbers(in, 1, v)) return 2;
            const double out[2] = {sdlsq::softplus(v[0]), sdlsq::sigmoid(v[0])};
            print_numbers("helpers", out, 2);
        } else {
            return 2;
        }
    }
    std::printf("end\n");
    return 0;
}
