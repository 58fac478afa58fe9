#define CIAO_T double
#include "colsq_launch.inc"
