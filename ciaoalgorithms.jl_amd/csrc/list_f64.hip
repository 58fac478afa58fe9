#define CIAO_T double
#include "list_launch.inc"
