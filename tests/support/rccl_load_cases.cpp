// rccl_load_cases.cpp — a stand-alone program around ec3d_rccl_load (csrc/ec3d_rccl.cpp), for tests/test_rccl_load_host.py.
// Built together with csrc/ec3d_rccl.cpp under the address and undefined-behaviour sanitizers; needs no GPU.
//
//     rccl_load_cases <calls>
//
// calls ec3d_rccl_load <calls> times with EC3D_RCCL_LIB as the environment has it (the second call of a failing case takes
// the cached-error branch) and prints one line per call:
//     call <i> EC3D_RCCL_LIB=<value | (unset)> loaded path=<file>
//     call <i> EC3D_RCCL_LIB=<value | (unset)> error <message>
// Exit status 0 whatever the loader answered: an answer is what is tested, not which.
#include "ec3d_rccl.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    const int calls = argc > 1 ? atoi(argv[1]) : 1;
    const char *named = getenv("EC3D_RCCL_LIB");
    const ec3d_rccl_api *first = nullptr;
    for (int i = 0; i < calls; i++) {
        std::string why;
        const ec3d_rccl_api *api = ec3d_rccl_load(why);
        if (api) {
            if (!why.empty() || (i && api != first)) return 3; // a table comes without a reason, and is the same table again
            if (!api->GetUniqueId || !api->Send || !api->Recv || !api->AllGather) return 4;
            printf("call %d EC3D_RCCL_LIB=%s loaded path=%s\n", i, named ? named : "(unset)", api->path);
        } else {
            if (why.empty()) return 5; // a refusal comes with its reason
            printf("call %d EC3D_RCCL_LIB=%s error %s\n", i, named ? named : "(unset)", why.c_str());
        }
        if (!i) first = api;
    }
    return 0;
}
