#define CIAO_T float
#include "rowsq_launch.inc"
