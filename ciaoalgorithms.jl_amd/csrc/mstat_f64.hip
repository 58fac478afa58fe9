#define CIAO_T double
#include "mstat_launch.inc"
