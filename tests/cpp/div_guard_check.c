// What the range guards of the exact-division fast path protect (ammsb_dev.h "exact division", where the bounds and the
// fast / slow quotients of every update_phi and beta-gradient form are stated once): reads binary32 (x, d)
// operand pairs from a file and counts the quotients that the two unguarded tails get wrong against IEEE `x / d`:
//   three instructions (Markstein), y = RN(1 / d):   q0 = x*y; rem = fma(-d, q0, x); q = fma(rem, y, q0)
//   five instructions, from a reciprocal seed within 1 ulp of RN(1 / d), refined once (as div_check.c does):
//     e = fma(-d, y0, 1); r = fma(e, y0, y0); q0 = x*r; e1 = fma(-d, q0, x); q1 = fma(e1, r, q0); e2 = fma(-d, q1, x);
//     q = fma(e2, r, q1)                       -- a pair counts once if any of the three seeds misses
// Two NaNs count as equal.  Build: gcc -O2 -ffp-contract=off div_guard_check.c -lm
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
static inline float asf(uint32_t u){float f;memcpy(&f,&u,4);return f;}
static inline uint32_t asu(float f){uint32_t u;memcpy(&u,&f,4);return u;}
static inline int same(float a,float b){return (isnan(a)&&isnan(b))||asu(a)==asu(b);}
int main(int argc,char**argv){
  if(argc<2){fprintf(stderr,"usage: %s pairs.bin\n",argv[0]);return 2;}
  FILE*f=fopen(argv[1],"rb");
  if(!f){perror(argv[1]);return 2;}
  long n=0,bad3=0,bad5=0;
  float p[2];
  while(fread(p,sizeof(float),2,f)==2){
    volatile float x=p[0],d=p[1];
    const float want=x/d;
    const float y=1.0f/d;
    {
      const float q0=x*y; const float rem=fmaf(-d,q0,x); const float q=fmaf(rem,y,q0);
      if(!same(q,want)) ++bad3;
    }
    int miss=0;
    for(int dl=-1;dl<=1;++dl){
      const float y0=asf(asu(y)+dl);
      const float e=fmaf(-d,y0,1.0f); const float r=fmaf(e,y0,y0);
      const float q0=x*r; const float e1=fmaf(-d,q0,x); const float q1=fmaf(e1,r,q0);
      const float e2=fmaf(-d,q1,x); const float q=fmaf(e2,r,q1);
      if(!same(q,want)) miss=1;
    }
    bad5+=miss;
    ++n;
  }
  fclose(f);
  printf("pairs %ld tail3 %ld tail5 %ld\n",n,bad3,bad5);
  return 0;
}
