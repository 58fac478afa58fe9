#define CIAO_T float
#include "colsq_launch.inc"
