#define CIAO_T double
#include "colmom_launch.inc"
