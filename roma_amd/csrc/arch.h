// Private to model.hip / model_weights.hip: the architecture tables of the state dict and of the schedule.
#pragma once

namespace roma {

static const int VGG_IDX[12] = {0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36};
static const int VGG_CH[12] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512};
static const char* SCALES[5] = {"16", "8", "4", "2", "1"};
static const int SCALE_INT[5] = {16, 8, 4, 2, 1};
static const int PROJ_CIN[5] = {1024, 512, 256, 128, 64};
static const int PROJ_COUT[5] = {512, 512, 256, 64, 9};
static const int REF_EMB[5] = {128, 64, 32, 16, 6};
static const int REF_RAD[5] = {7, 3, 2, 0, 0};

}  // namespace roma
