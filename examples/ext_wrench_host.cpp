// ext_wrench_host.cpp -- the single-configuration external-wrench forms on the embedded FR3, no
// GPU: qdd = fd_ext(q, qd, tau, fext), then rnea_ext(q, qd, qdd, fext) must give tau back, and a
// zero wrench must reproduce multibody_rnea.  Stand-alone so the host code can run under
// AddressSanitizer / UBSan: build the library's host objects and this file with
// -fsanitize=address,undefined and run it on the CPU.
//
//   g++ -O1 -std=c++17 -Iinclude examples/ext_wrench_host.cpp -Lrigidbody-rs_amd -lrigidbody_bindings
#include <cmath>
#include <cstdio>
#include <vector>

#include "rigidbody.h"
#include "rigidbody_batch.h"

int main() {
    Multibody *mb = multibody_new();
    if (!mb) {
        std::fprintf(stderr, "multibody_new: %s\n", rb_last_error());
        return 1;
    }
    const int n = multibody_dof(mb);
    std::vector<double> q(n), qd(n), tau(n), fext(6 * n), qdd(n), back(n), zero(6 * n, 0.0);
    double worst = 0.0;
    for (int trial = 0; trial < 50; ++trial) {
        for (int j = 0; j < n; ++j) {
            q[j] = 0.3 * std::sin(1.0 + trial + 0.7 * j);
            qd[j] = 0.5 * std::cos(2.0 + trial - 0.3 * j);
            tau[j] = 4.0 * std::sin(0.1 * trial + j);
        }
        for (int r = 0; r < 6 * n; ++r) fext[r] = (r % 6 < 3 ? 20.0 : 5.0) * std::sin(0.37 * r + trial);
        if (multibody_fd_ext(mb, q.data(), qd.data(), tau.data(), fext.data(), qdd.data()) != RB_OK ||
            multibody_rnea_ext(mb, q.data(), qd.data(), qdd.data(), fext.data(), back.data()) != RB_OK) {
            std::fprintf(stderr, "ext call failed: %s\n", rb_last_error());
            return 1;
        }
        for (int j = 0; j < n; ++j) worst = std::fmax(worst, std::fabs(back[j] - tau[j]) / (1.0 + std::fabs(tau[j])));
        if (multibody_rnea_ext(mb, q.data(), qd.data(), qdd.data(), zero.data(), back.data()) != RB_OK) return 1;
        double *plain = multibody_rnea(mb, q.data(), qd.data(), qdd.data());
        if (!plain) return 1;
        for (int j = 0; j < n; ++j)
            if (plain[j] != back[j]) {
                std::fprintf(stderr, "zero wrench differs from rnea at joint %d\n", j);
                return 1;
            }
        multibody_result_free(plain);
    }
    multibody_free(mb);
    std::printf("ext_wrench_host ok: round-trip residual %.3e\n", worst);
    return worst <= 1e-8 ? 0 : 1;
}
