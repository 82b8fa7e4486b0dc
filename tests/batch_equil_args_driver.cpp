// Stand-alone driver for batch_args::elements_step (csrc/batch_args.h), the chunk rule of the equilibration's elementwise kernels; built
// with AddressSanitizer and UBSan and run directly by tests/test_batched_equil_cpu.py.  One question per line on stdin:
//   step <max_launch> <per>            -> the step
//   cover <batch> <max_launch> <per>   -> the chunks b0:count of the batch, and "ok" when each holds fewer than 2^31 elements
#include "../mixed-precision_lu_factorization_amd/csrc/batch_args.h"
#include <iostream>
#include <sstream>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "step") {
            int64_t max_launch, per;
            in >> max_launch >> per;
            std::cout << batch_args::elements_step(max_launch, per) << "\n";
        } else if (what == "cover") {
            int64_t batch, max_launch, per;
            in >> batch >> max_launch >> per;
            bool ok = true;
            int64_t next = 0;
            batch_args::chunks(batch, batch_args::elements_step(max_launch, per), [&](int64_t b0, int64_t nb) {
                std::cout << b0 << ":" << nb << " ";
                ok = ok && b0 == next && nb >= 1 && nb <= max_launch && (nb == 1 || nb * per < ((int64_t)1 << 31));
                next = b0 + nb;
                return 0;
            });
            std::cout << (ok && next == batch ? "ok" : "bad") << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
