#define CIAO_T double
#include "rowsq_launch.inc"
