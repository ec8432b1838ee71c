// plan_dump -- what a configuration launches, without a device: the graph of build_layers, one plan_forward, and the layer table's rows
// (name <TAB> kernel label <TAB> launches) as idc_layer_info_get labels them.  The persistent kwave chain is an execution-time decision and
// does not show here: a handle's table agrees with this one after a forward with idc_set_option("kwave_chain", 0).
//   plan_dump PRECISION FLAGS H W MAX_BATCH N [name=value ...]
//   PRECISION: fp32 bf16 bf16x3 bf16x6 fp16x3 fp16; FLAGS: the IDC_FLAG_* bits as a number; name=value: idc_set_option's, and tile_policy / splitk_policy
// Build: make -C interactive_deep_colorization_amd/csrc plan_dump (links the built library; makes no HIP runtime call).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "idc_engine.h"

int main(int argc, char** argv) {
    static const char* const kPrecisions[] = {"fp32", "bf16", "bf16x3", "bf16x6", "fp16x3", "fp16"};
    int precision = -1;
    for (int i = 0; argc >= 7 && i < 6; ++i)
        if (strcmp(argv[1], kPrecisions[i]) == 0) precision = i;
    if (precision < 0) {
        fprintf(stderr, "usage: plan_dump fp32|bf16|bf16x3|bf16x6|fp16x3|fp16 FLAGS H W MAX_BATCH N [name=value ...]\n");
        return 2;
    }
    PlanEnv env;
    env.precision = precision;
    env.flags = (unsigned)strtoul(argv[2], nullptr, 0);
    env.H = atoi(argv[3]); env.W = atoi(argv[4]); env.max_batch = atoi(argv[5]); env.n = atoi(argv[6]);
    if (env.H <= 0 || env.W <= 0 || env.H % 8 || env.W % 8 || env.n <= 0 || env.n > env.max_batch) {
        fprintf(stderr, "plan_dump: H and W must be positive multiples of 8, 1 <= N <= MAX_BATCH\n");
        return 2;
    }
    for (int i = 7; i < argc; ++i) {
        char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "plan_dump: '%s' is not name=value\n", argv[i]); return 2; }
        *eq = 0;
        const int value = atoi(eq + 1);
        const int rc = strcmp(argv[i], "tile_policy") == 0 ? idc_set_tile_policy(value) :
                       strcmp(argv[i], "splitk_policy") == 0 ? idc_set_splitk_policy(value) : idc_set_option(argv[i], value);
        if (rc) { fprintf(stderr, "plan_dump: %s\n", idc_last_error(nullptr)); return 2; }
    }
    const BlobPlan blob = make_blob_plan(precision, env.flags);
    std::vector<Tensor> tensors;
    std::vector<Layer> layers;
    std::string err;
    int rc = build_layers(blob, precision, env.H, env.W, env.max_batch, tensors, layers, &err);
    env.t_conv10_2 = find_tensor(tensors, "conv10_2");
    env.t_conv4_3 = find_tensor(tensors, "conv4_3");
    if (rc == IDC_OK) rc = plan_forward(layers, tensors, env, &err);
    if (rc) { fprintf(stderr, "plan_dump: %s\n", err.c_str()); return 1; }
    for (int row = 0; row < (int)layers.size() + 3; ++row) {
        idc_layer_info info;
        layer_row(layers, tensors, precision, env.flags, env.H, env.W, row, &info);
        printf("%s\t%s\t%d\n", info.name, info.kernel, info.launches);
    }
    return 0;
}
