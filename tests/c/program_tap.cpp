// CPU: the h-space tap of the U-Net program (loco-edit_amd/csrc/program.hip).  Reads "<name> <hex bytes of loco_unet_cfg>" lines like
// program_check.cpp and prints per config
//   TAP <name> h_t= h_last_op= n_h= op=<name of op h_last_op> out=<its output tensor> shape=C,H,W next=<name of the op behind it> cat_a_of_next_in=<0|1>
// (h_t = -1 for a network without a tap), or "TAP <name> rc=<code>" for a refused configuration.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../../loco-edit_amd/csrc/program.h"

using namespace loco;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: program_tap <configs>\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string name, hex;
    while (f >> name >> hex) {
        loco_unet_cfg cfg;
        if (hex.size() != 2 * sizeof(cfg)) { printf("TAP %s rc=-9\n", name.c_str()); continue; }
        for (size_t i = 0; i < sizeof(cfg); ++i) ((unsigned char*)&cfg)[i] = (unsigned char)strtol(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        Program p;
        std::string err;
        const int rc = build_program(cfg, &p, &err);
        if (rc) { printf("TAP %s rc=%d\n", name.c_str(), rc); continue; }
        if (p.h_t < 0) { printf("TAP %s h_t=%d h_last_op=%d n_h=%d\n", name.c_str(), p.h_t, p.h_last_op, p.n_h); continue; }
        const OpPlan& op = p.ops[p.h_last_op];
        const OpPlan& nx = p.ops[p.h_last_op + 1];
        const TensPlan& t = p.tens[p.h_t];
        printf("TAP %s h_t=%d h_last_op=%d n_h=%d op=%s out=%d shape=%d,%d,%d next=%s cat_a_of_next_in=%d\n", name.c_str(), p.h_t, p.h_last_op,
               p.n_h, op.name.c_str(), op.out, t.C, t.H, t.W, nx.name.c_str(), (int)(p.tens[nx.in].cat_a == p.h_t));
    }
    return 0;
}
