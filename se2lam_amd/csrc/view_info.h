// The arithmetic a new observation needs (DLT, se3map, calcSE3toXYZInfo, acceptNewObserve) is shared with the host mirror
// include/se2lam_amd/FindCorrespd.h and therefore lives under include/, like VocabularyTrain.h; the kernels take it from here.
#pragma once
#include "../../include/se2lam_amd/view_info.h"
