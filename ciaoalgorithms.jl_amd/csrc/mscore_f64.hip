#define CIAO_T double
#include "mscore_launch.inc"
