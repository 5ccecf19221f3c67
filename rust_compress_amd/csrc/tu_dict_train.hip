// tu_dict_train.hip -- dictionary training: the batched cover trainer behind rcx_dict_train_batch.
#include "rcx_tu.h"
#include "k_dict_train.hip"

int rcx_tu_dict_train(hipStream_t s, rcx_kargs& k, const rcx_train_plan& plan, std::string& err) { return launch_dict_train(s, k, plan, err); }
